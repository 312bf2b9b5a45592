"""-A after -c on the host: cl_induced_cyclic_maf == output_maf(induced_cyclic_pairwise_alignment(...)) (src/alignment.cpp:229-904) of the
unmodified reference, on the cyclised graph of its own -c -A run (tests/golden/make_induced_maf.py), on hand-made cyclic graphs, and, where
the reference is built, live on small random -c inputs."""
import gzip
import hashlib
import json
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from centrolign_amd import capi
from tests import helpers as H
from tests.test_gpu_induced_pairs import path_graph

REF_CLI = os.path.join(os.path.dirname(H.GOLDEN), "..", "oracle", "_ref", "ref_cli")


def maf(g, a, b, names):
    return capi.induced_cyclic_maf(g, a, b, names[a], names[b])


def blocks(text):
    """[(start1, size1, row1, start2, size2, row2)] of a MAF text"""
    out = []
    for blk in text.decode().split("\n\na\n")[1:]:
        s1, s2 = [ln.split("\t") for ln in blk.strip("\n").split("\n")]
        out.append((int(s1[2]), int(s1[3]), s1[5], int(s2[2]), int(s2[3]), s2[5]))
    return out


@pytest.mark.parametrize("case,gfa", [("induced_16x12k", "cyclize_16x12k"), ("induced_nobond", None)])
def test_cyclic_maf_matches_the_reference_on_its_own_graph(case, gfa):
    """every pair of the reference's -c -A run, by digest.  The MAF reads path steps and labels only, not node-id values, so the graph read
    back from the GFA the reference printed (other node ids) gives the same text"""
    want = json.load(open(os.path.join(H.GOLDEN, case + ".json")))
    if gfa:
        assert json.load(open(os.path.join(H.GOLDEN, gfa + ".json")))["gfa"]["sha256"] == want["gfa"]["sha256"]
        text = gzip.decompress(open(os.path.join(H.GOLDEN, gfa + ".gfa.gz"), "rb").read())
    else:
        text = gzip.decompress(open(os.path.join(H.GOLDEN, case + ".gfa.gz"), "rb").read())
    assert hashlib.sha256(text).hexdigest() == want["gfa"]["sha256"]
    g, names = capi.read_gfa(text, add_sentinels=False)
    kept = json.loads(gzip.decompress(open(os.path.join(H.GOLDEN, case + "_maf.json.gz"), "rb").read()))
    n = 0
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            f = "%s_%s.maf" % (names[a].replace("/", "_"), names[b].replace("/", "_"))
            got = maf(g, a, b, names)
            if f in kept:
                assert got.decode() == kept[f], f
            assert hashlib.sha256(got).hexdigest() == want["files"][f]["sha256"], f
            n += 1
    assert n == sum(f.endswith(".maf") for f in want["files"])


def test_cyclic_maf_branches_on_hand_made_graphs():
    labels = [0, 1, 2, 3] * 8 + [5, 6, 4]
    g = path_graph(labels, [
        [0, 1, 2, 3, 4, 5, 6, 7],
        [0, 1, 2, 3, 4, 5, 6, 7],
        [10, 11, 12],                       # nothing in common with path 0
        [3],                                # one step
        [32, 33, 34, 0, 1],                 # labels above 4, and N
        [0, 1, 2, 3, 0, 1, 2, 3, 4, 5],     # a repeat: blocks may not merge across it
        [8, 9, 8, 9, 8],                    # dangling insertions split at each repeat
    ])
    names = ["p%d" % i for i in range(7)]
    # identical paths: one block
    b = blocks(maf(g, 0, 1, names))
    assert b == [(0, 8, "ACGTACGT", 0, 8, "ACGTACGT")]
    assert maf(g, 0, 1, names).startswith(b"track name=p0_vs_p1_induced\n##maf version=1\n")
    # empty LCS: only dangling blocks, the empty side at the path's length
    b = blocks(maf(g, 0, 2, names))
    assert b == [(0, 8, "ACGTACGT", 3, 0, "--------"), (8, 0, "---", 0, 3, "GTA")]
    # a path of one step: its match, extended over the whole of the other path
    assert blocks(maf(g, 3, 0, names)) == [(0, 1, "---T----", 0, 8, "ACGTACGT")]
    # labels above 4 written as raw bytes, 4 as N
    b = blocks(maf(g, 4, 0, names))
    assert any("\x05\x06N" in x[2] for x in b)
    # every step of both paths lies in exactly one block, and no block repeats a node
    for p, q in [(5, 0), (0, 5), (6, 0), (5, 6), (6, 6), (5, 5)]:
        bl = blocks(maf(g, p, q, names))
        n1 = int(g.path_off[p + 1] - g.path_off[p])
        n2 = int(g.path_off[q + 1] - g.path_off[q])
        assert sum(x[1] for x in bl) == n1 and sum(x[4] for x in bl) == n2
        for x in bl:
            if x[1]:
                steps = g.path_nodes[int(g.path_off[p]) + x[0]:int(g.path_off[p]) + x[0] + x[1]]
                assert len(set(steps.tolist())) == len(steps)
    # the repeat of path 5 keeps its two copies in separate blocks against path 0
    assert len([x for x in blocks(maf(g, 5, 0, names)) if x[1]]) >= 2
    # path 6 against an unrelated path: one dangling block per stretch without a repeat (8 9 | 8 9 | 8)
    assert [x[1] for x in blocks(maf(g, 6, 2, names)) if x[1]] == [2, 2, 1]
    with pytest.raises(capi.ClError):
        capi.induced_cyclic_maf(g, 0, 7, "a", "b")


@pytest.mark.skipif(not os.path.exists(REF_CLI), reason="the compiled reference is not built here")
def test_cyclic_maf_matches_the_reference_live():
    """small random -c -A runs of the reference: each .maf recomputed from the GFA that run printed (inputs the reference itself dies on,
    DESIGN.md §11, are passed over)"""
    from centrolign_amd import msa, synth
    rng = random.Random(5)
    done = 0
    for case in range(8):
        n = rng.randint(3, 5)
        names = ["r%d" % i for i in range(n)]
        seqs = synth.tandem_dup_sequences(100 + case, rng.randint(2500, 4000), n, 600, carriers=[0, n - 1])
        d = tempfile.mkdtemp(prefix="induced_live_")
        synth.write_fasta(os.path.join(d, "in.fa"), seqs, names)
        open(os.path.join(d, "t.nwk"), "w").write(msa.newick(msa.balanced_tree(names)) + ";\n")
        if subprocess.call(["bash", "-c", "cd %s && %s in.fa t.nwk - out.gfa 0 1 0 's:all_pairs_prefix=pw;b:cyclize_tandem_duplications=1;"
                            "i:min_cyclizing_length=400;i:max_num_match_pairs=20000' > ref.log 2>&1" % (d, os.path.abspath(REF_CLI))]):
            continue
        done += 1
        g, pn = capi.read_gfa(open(os.path.join(d, "out.gfa"), "rb").read(), add_sentinels=False)
        for a in range(n):
            for b in range(a + 1, n):
                assert maf(g, a, b, pn) == open(os.path.join(d, "pw_%s_%s.maf" % (pn[a], pn[b])), "rb").read(), (case, a, b)
        if done == 3:
            break
    assert done >= 2
