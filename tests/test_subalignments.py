"""-s and --bond-prefix on the host: cl_bond_alignment_cigar against the unmodified reference's bond CIGAR files and a Python restatement of
Core::output_bond_alignment (include/centrolign/core.hpp:426-500); the '# sequence set' headers of its -s files against the plan
(Execution::leaf_descendents, src/execution.cpp:163-187); the new entry points in the ABI.  Goldens: tests/golden/make_subalignments.py."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

from centrolign_amd import capi
from tests import helpers as H
from tests.golden import make_subalignments as ms

GAP = 2 ** 64 - 1
WANT = json.load(open(os.path.join(H.GOLDEN, "subalignments.json")))


def as_nodes(p):
    """path positions of PREFIX_bonds.txt (-1: gap) -> node ids of the leaf graph (UINT64_MAX: gap)"""
    return [(GAP if a < 0 else int(a), GAP if b < 0 else int(b)) for a, b in np.asarray(p).reshape(-1, 2).tolist()]


def py_explicit_cigar(labels, pairs):
    out, run, op = [], 0, None
    for a, b in pairs:
        o = "I" if a == GAP else "D" if b == GAP else "=" if labels[a] == labels[b] else "X"
        if o == op:
            run += 1
            continue
        if run:
            out.append("%d%s" % (run, op))
        run, op = 1, o
    if run:
        out.append("%d%s" % (run, op))
    return "".join(out)


def py_bond_cigar(labels, path, aln):
    """Core::output_bond_alignment, line by line"""
    first1 = next((a for a, _ in aln if a != GAP), None)
    first2 = next((b for _, b in aln if b != GAP), None)
    last1 = next((a for a, _ in reversed(aln) if a != GAP), None)
    last2 = next((b for _, b in reversed(aln) if b != GAP), None)
    if first1 is None:
        return b"\n"
    padded = []
    for v in path:
        if v == first1:
            break
        padded.append((v, GAP))
    for v in path:
        if v == first2:
            break
        padded.append((GAP, v))
    padded += list(aln)
    lag = []
    for v in reversed(path):
        if v == last2:
            break
        lag.append((GAP, v))
    for v in reversed(path):
        if v == last1:
            break
        lag.append((v, GAP))
    padded += lag[::-1]
    return (py_explicit_cigar(labels, padded) + "\n").encode()


def cyclize_leaves():
    from tests.golden import make_cyclize_wide as mcw
    names, seqs, _ = mcw.workload("cyclize_16x12k")
    return dict(zip(names, seqs))


def test_leaf_graph_numbers_bases_as_path_positions():
    """the bond alignments are path positions, the reference writes node ids: on a leaf graph they are the same numbers"""
    g = capi.leaf_graph("ACGTNACGTT")
    assert g.path_off.tolist() == [0, 10] and g.path_nodes.tolist() == list(range(10))
    assert {g.src_id, g.snk_id} == {10, 11}


def test_bond_cigars_match_the_reference_files():
    """every PREFIX_<seq>_cigar_<k>.txt of the reference's -c --bond-prefix run, from its PREFIX_bonds.txt and the leaf graphs"""
    want = WANT["sub_cyclize"]
    assert want["gfa_is_cyclize_16x12k"] and want["malloc_perturb"] is not None
    bonds = ms.load_bonds()
    assert hashlib.sha256(ms.bonds_text(bonds)).hexdigest() == want["files"]["sp_bonds.txt"]["sha256"]
    seqs = cyclize_leaves()
    graphs = {n: capi.leaf_graph(s) for n, s in seqs.items()}
    count, got = {}, {}
    for name, p in bonds:
        k = count.get(name, 0)
        count[name] = k + 1
        got["bd_%s_cigar_%d.txt" % (name, k)] = capi.bond_alignment_cigar(graphs[name], as_nodes(p))
    assert sorted(got) == sorted(f for f in want["files"] if f.startswith("bd_"))
    for f, text in sorted(got.items()):
        assert hashlib.sha256(text).hexdigest() == want["files"][f]["sha256"], f
    g = graphs["c00"]
    labels, path = g.label, g.path_nodes.tolist()
    for name, p in bonds[:6]:   # (and the restatement agrees)
        if name == "c00":
            assert capi.bond_alignment_cigar(g, as_nodes(p)) == py_bond_cigar(labels, path, as_nodes(p))


@pytest.mark.parametrize("aln", [
    [],                                          # empty: the line end alone
    [(GAP, 3), (GAP, 4)],                        # no node on side 1: the line end alone
    [(2, GAP), (3, GAP), (4, GAP)],              # no node on side 2: the whole path as insertions in front and behind
    [(0, 5), (1, 6), (2, 7)],                    # side 1 at the path's start
    [(3, 0), (4, 1), (5, GAP), (6, 2)],          # side 2 at the path's start
    [(7, 9), (GAP, 10), (8, 11)],                # side 2 at the path's end
    [(0, 11), (11, 0)],                          # both sides at both ends
    [(GAP, 2), (3, 4), (5, GAP), (GAP, 9), (6, 10), (7, GAP)],
])
def test_bond_cigar_hand_made(aln):
    seq = "ACGTACGTTACG"
    g = capi.leaf_graph(seq)
    assert capi.bond_alignment_cigar(g, aln) == py_bond_cigar(g.label, g.path_nodes.tolist(), aln)


def test_bond_cigar_rejects_a_bad_path():
    g = capi.leaf_graph("ACGT")
    with pytest.raises(capi.ClError):
        capi.bond_alignment_cigar(g, [(0, 1)], path=1)


def py_headers(names, newick, removed=()):
    """the two '# sequence set' lists of every merge the run computes, in plan order: each child's leaves right to left.  removed: the leaf
    sets whose -S files a restart does not find (every other subproblem file exists)"""
    leaves, merges = capi.msa_plan(newick, names)
    sets = [[names[s]] for s in leaves]
    for a, b in merges:
        sets.append(sets[a] + sets[b])
    done = [False] * len(sets)
    if removed is not None and removed != ():
        gone = {tuple(sorted(r)) for r in removed}
        for k in reversed(range(len(merges))):   # Execution::restart: from the root down, what is loaded makes its subtree unnecessary
            slot = len(leaves) + k
            if not done[slot] and tuple(sorted(sets[slot])) not in gone:
                done[slot] = True
            if done[slot]:
                for c in merges[k]:
                    done[c] = True
    return [[sets[a][::-1], sets[b][::-1]] for k, (a, b) in enumerate(merges) if not done[len(leaves) + k]]


@pytest.mark.parametrize("case", ["sub_nobond", "sub_unbalanced", "sub_two", "sub_restart", "sub_cyclize"])
def test_sequence_set_headers_follow_the_plan(case):
    want = WANT[case]
    assert py_headers(want["names"], want["newick"], want.get("removed", ())) == want["headers"]


def test_unbalanced_case_prunes_and_binarises():
    """the unbalanced golden's tree has a leaf that is not in the FASTA and a node with three children"""
    want = WANT["sub_unbalanced"]
    assert "gone" in want["newick"] and "gone" not in want["names"]
    leaves, merges = capi.msa_plan(want["newick"], want["names"])
    assert len(leaves) == len(want["names"]) and len(merges) == len(want["names"]) - 1 == len(want["headers"])


def test_small_goldens_are_consistent():
    """the kept texts are the files the digests describe, and every -s file is blocks of well-formed lines"""
    import gzip
    texts = json.loads(gzip.decompress(open(os.path.join(H.GOLDEN, "subalignments_text.json.gz"), "rb").read()))
    for case, files in texts.items():
        for f, t in files.items():
            assert hashlib.sha256(t.encode("latin-1")).hexdigest() == WANT[case]["files"][f]["sha256"]
    sub = texts["sub_two"]["sub.txt"]
    body = sub.split("# alignment\n", 1)[1]
    line = re.compile(r"^(-\t-\t-|t0\t\d+\t[ACGTN])\t(-\t-\t-|t1\t\d+\t[ACGTN])$")
    assert all(line.match(ln) for ln in body.split("\n")[:-1])


def test_new_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(os.path.dirname(H.GOLDEN), "..", "include", "centrolign_amd.h")).read()
    for sym in ("cl_subalignment_text", "cl_bond_alignment_cigar"):
        assert re.search(r"\bint %s\(" % sym, hdr), sym
        assert sym in capi.EXPORTED_SYMBOLS
        getattr(capi.load_library(), sym)
    for field in ("subalignments_path", "bonds_prefix", "force_gfa_output"):
        assert field in hdr and field in [f for f, _ in capi.MsaParams._fields_]
    assert [f for f, _ in capi.MsaParams._fields_][-3:] == ["subalignments_path", "bonds_prefix", "force_gfa_output"]
    lib = capi.load_library()
    assert lib.cl_abi_version() == capi.ABI_VERSION
    p = capi.MsaParams()
    lib.cl_msa_params_default(ctypes.byref(p))
    assert p.subalignments_path is None and p.bonds_prefix is None and p.force_gfa_output == 0
