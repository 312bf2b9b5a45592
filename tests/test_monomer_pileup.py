"""Monomer pileups, consensus and template refinement (cl_monomer_pileup_host, cl_monomer_consensus, cl_monomer_templates_refine_host,
cl_monomer_seed_templates, the two text writers, the CLI's --monomers-rounds family), without a GPU: the host definition against a restatement
that shares no code with the library (`align`: one numpy row of G at a time, the walk back in Python; `restated_pileup`: the classes and the
counts from lists of aligned bases), the hand cases of the definition, the score invariant, every consensus rule, the recovery, low-depth and seed
runs, the text byte for byte, every refused argument, the ABI and every refusal of the command line, which comes before a device is opened.
tests/test_gpu_monomer_pileup.py holds the device path against the host."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_monomers import BIN, ROOT, SCORE_SETS, params, random_case, revcomp

_CODE = {c: k for k, c in enumerate("ACGT")}
_CODE.update({c.lower(): k for c, k in list(_CODE.items())})
PILEUP_HEADER = "monomer\tposition\tbase\tA\tC\tG\tT\tother\tdeleted\tins_A\tins_C\tins_G\tins_T\tins_other\n"


def code(c):
    return _CODE.get(c, 4)


def align(x, b, scores):
    """(score, per column the block base or None, per slot the inserted bases in the block's order) by the definition's recurrence and walk"""
    match, mismatch, ins, dele = scores
    n, L = len(x), len(b)
    xc = [code(c) for c in x]
    bc = np.array([code(c) if code(c) < 4 else 5 for c in b], np.int64)
    j = np.arange(L + 1, dtype=np.int64)
    G = np.zeros((n + 1, L + 1), np.int64)
    G[0] = j * dele
    for i in range(1, n + 1):
        T = np.empty(L + 1, np.int64)
        T[0] = i * ins
        T[1:] = np.maximum(G[i - 1, :-1] + np.where(bc == xc[i - 1], match, mismatch), G[i - 1, 1:] + ins)
        G[i] = np.maximum.accumulate(T - j * dele) + j * dele   # the deletions of a row in one pass
    cols, slots = [None] * L, [[] for _ in range(L + 1)]
    i, k = n, L
    while i > 0 or k > 0:
        if i > 0 and k > 0 and G[i, k] == G[i - 1, k - 1] + (match if bc[k - 1] == xc[i - 1] else mismatch):
            cols[k - 1] = x[i - 1]
            i, k = i - 1, k - 1
        elif i > 0 and G[i, k] == G[i - 1, k] + ins:
            slots[k].insert(0, x[i - 1])
            i -= 1
        else:
            k -= 1
    return int(G[n, L]), cols, slots


def restated_pileup(seqs, templates, blocks, scores=(1, -1, -1, -1), strands=1, least_share=0):
    """the pileup dict of capi.monomer_pileup_host, from the blocks (sequence, start, end, monomer, score, flags)"""
    M = len(templates)
    col_off = np.concatenate([[0], np.cumsum([len(t) for t in templates])]).astype(np.uint64)
    total = int(col_off[M])
    out = {"n_templates": M, "col_off": col_off, "columns": np.zeros((total, 6), np.uint32), "slots": np.zeros((total + M, 5), np.uint32),
           "score_sum": np.zeros(M, np.int64)}
    for name in ("used", "partial", "long_", "weak"):
        out[name] = np.zeros(M, np.uint64)
    comp = [3, 2, 1, 0, 4]
    for s, start, end, mono, score, flags in blocks:
        m, minus = mono % M, mono >= M
        L = len(templates[m])
        if flags != 0:
            out["partial"][m] += 1
        elif end - start > 2 * L:
            out["long_"][m] += 1
        elif score * 1000 < least_share * scores[0] * L:
            out["weak"][m] += 1
        else:
            out["used"][m] += 1
            g, cols, slots = align(seqs[s][start:end], revcomp(templates[m]) if minus else templates[m], scores)
            out["score_sum"][m] += g
            c0 = int(col_off[m])
            for k, base in enumerate(cols):
                if minus:
                    out["columns"][c0 + L - 1 - k, 5 if base is None else comp[code(base)]] += 1
                else:
                    out["columns"][c0 + k, 5 if base is None else code(base)] += 1
            for k, inserted in enumerate(slots):
                if inserted and minus:
                    out["slots"][c0 + m + L - k, comp[code(inserted[-1])]] += 1
                elif inserted:
                    out["slots"][c0 + m + k, code(inserted[0])] += 1
    return out


def same_pileup(got, want):
    for name in ("col_off", "columns", "slots", "used", "partial", "long_", "weak", "score_sum"):
        assert np.array_equal(got[name], want[name]), (name, got[name].tolist()[:40], want[name].tolist()[:40])
    assert got["n_templates"] == want["n_templates"]


def block_list(dec):
    return [tuple(int(v) for v in b) for b in dec["blocks"].tolist()]


def dec_of(blocks, n_seq):
    """a decomposition dict from hand-written blocks"""
    arr = np.array(blocks, capi.MONOMER_BLOCK) if blocks else np.zeros(0, capi.MONOMER_BLOCK)
    return {"n_seq": n_seq, "n_blocks": len(arr), "n_problems": n_seq, "seq_off": np.searchsorted(arr["sequence"], np.arange(n_seq + 1)).astype(np.uint64), "blocks": arr}


def check_host(seqs, templates, dec, scores=(1, -1, -1, -1), strands=1, least_share=0):
    want = restated_pileup(seqs, templates, block_list(dec), scores, strands, least_share)
    got = capi.monomer_pileup_host(seqs, templates, dec, least_share, **params(scores, strands=strands))
    same_pileup(got, want)
    assert got["align_ms"] == 0 and got["count_ms"] == 0
    return got


# ---------------------------------------------------------------- the hand cases of the definition ---------------------------------------------
HAND = [("AA", "A", 0, [None, "A"], {}), ("A", "AA", 0, ["A"], {0: "A"}), ("AAAA", "AA", 0, [None, None, "A", "A"], {}), ("ACGT", "AGT", 2, ["A", None, "G", "T"], {}),
        ("ACGT", "ACCGT", 3, ["A", "C", "G", "T"], {1: "C"}), ("AC", "CA", -1, [None, "C"], {2: "A"}), ("ACGT", "NNNN", -4, ["N"] * 4, {})]


@pytest.mark.parametrize("template,block,score,cols,slots", HAND)
def test_hand_cases(template, block, score, cols, slots):
    g, got_cols, got_slots = align(block, template, (1, -1, -1, -1))
    assert (g, got_cols) == (score, cols) and {k: v[0] for k, v in enumerate(got_slots) if v} == slots   # the restatement itself
    dec = dec_of([(0, 0, len(block), 0, max(score, 0), 0)], 1)   # (a block whose own score is negative would be counted weak)
    got = check_host([block], [template], dec)
    assert got["score_sum"].tolist() == [score] and got["used"].tolist() == [1]
    want_cols = [[int(k == (5 if c is None else code(c))) for k in range(6)] for c in cols]
    want_slots = [[int(j in slots and k == code(slots[j])) for k in range(5)] for j in range(len(template) + 1)]
    assert got["columns"].tolist() == want_cols and got["slots"].tolist() == want_slots
    # the other strand: the same score; where the walk has a choice it is made in the reverse complement's order, so the counts may be mirrored
    mirrored = check_host([revcomp(block)], [template], dec_of([(0, 0, len(block), 1, max(score, 0), 0)], 1), strands=2)
    assert mirrored["score_sum"].tolist() == [score] and mirrored["columns"].sum() == got["columns"].sum()


def test_several_inserted_bases_record_the_first_in_template_order():
    got = check_host(["ACGTTTAC"], ["ACAC"], dec_of([(0, 0, 8, 0, 0, 0)], 1))
    assert got["slots"][2].tolist() == [0, 0, 1, 0, 0] and got["slots"].sum() == 1   # G of GTTT, in front of column 2
    minus = check_host([revcomp("ACGTTTAC")], ["ACAC"], dec_of([(0, 0, 8, 1, 0, 0)], 1), strands=2)
    assert np.array_equal(minus["slots"], got["slots"]) and np.array_equal(minus["columns"], got["columns"])


@pytest.mark.parametrize("scores", SCORE_SETS)
@pytest.mark.parametrize("strands", [1, 2])
def test_random_cases(scores, strands):
    for seed in (1, 2, 3):
        seq, templates = random_case(seed, n_templates=4, length=200)
        seqs = [seq, seq[50:120], ""]
        dec = capi.monomer_decompose_host(seqs, templates, **params(scores, chunk=0, strands=strands))
        got = check_host(seqs, templates, dec, scores, strands)
        assert got["used"].sum() > 10
        for share in (300, 1000):
            check_host(seqs, templates, dec, scores, strands, share)


def test_classes_in_their_order():
    """partial before long before weak; hand-written blocks, which the call takes like any other"""
    t = "ACGTACGTAC"
    seq = t * 4
    blocks = [(0, 0, 10, 0, 10, 1), (0, 0, 21, 0, 5, 3), (0, 0, 21, 0, 5, 0), (0, 0, 20, 0, 4, 0), (0, 0, 20, 0, 5, 0), (0, 10, 20, 0, 10, 0), (0, 20, 20, 0, 0, 0)]
    got = check_host([seq], [t], dec_of(blocks, 1), least_share=500)
    assert (got["partial"][0], got["long_"][0], got["weak"][0], got["used"][0]) == (2, 1, 2, 2)
    got = check_host([seq], [t], dec_of(blocks, 1))
    assert (got["partial"][0], got["long_"][0], got["weak"][0], got["used"][0]) == (2, 1, 0, 4)
    assert (got["columns"].sum(axis=1) == 4).all() and got["score_sum"][0] == 0 + 0 + 10 - 10   # (an empty block is all deletions)
    negative = check_host([seq], [t], dec_of([(0, 0, 10, 0, -1, 0)], 1))
    assert negative["weak"][0] == 1 and negative["used"][0] == 0   # score * 1000 >= 0 fails


# ---------------------------------------------------------------- the synthetic arrays ---------------------------------------------------------
@pytest.fixture(scope="module")
def hor():
    return synth.hor_sequences(5, 6000, 3), synth.hor_monomers(5)


@pytest.mark.parametrize("chunk,overlap", [(0, 0), (4096, 512)])
def test_score_invariant_and_column_sums(hor, chunk, overlap):
    seqs, templates = hor
    dec = capi.monomer_decompose_host(seqs, templates, chunk=chunk, overlap=overlap)
    assert dec["n_blocks"] == 129
    got = capi.monomer_pileup_host(seqs, templates, dec, chunk=chunk, overlap=overlap)
    used = [b for b in block_list(dec) if b[5] == 0 and b[2] - b[1] <= 2 * len(templates[b[3]])]
    assert len(used) == got["used"].sum() and got["long_"].sum() + got["partial"].sum() + len(used) == 129
    for s, start, end, m, score, _ in used:   # the global alignment's score is the decomposition's, block by block
        assert align(seqs[s][start:end], templates[m], (1, -1, -1, -1))[0] == score
    for m in range(12):
        assert got["score_sum"][m] == sum(b[4] for b in used if b[3] == m)
        assert (got["columns"][int(got["col_off"][m]):int(got["col_off"][m + 1])].sum(axis=1) == got["used"][m]).all()
    same_pileup(got, restated_pileup(seqs, templates, block_list(dec)))


def test_score_invariant_on_both_strands(hor):
    seqs, templates = hor
    flipped = [seqs[0], revcomp(seqs[1])]
    dec = capi.monomer_decompose_host(flipped, templates, chunk=0, strands=2)
    got = check_host(flipped, templates, dec, strands=2)
    used = [b for b in block_list(dec) if b[5] == 0 and b[2] - b[1] <= 2 * len(templates[b[3] % 12]) and b[4] >= 0]
    assert len(used) == got["used"].sum() > 80 and all(b[3] >= 12 for b in used if b[0] == 1) and got["score_sum"].sum() == sum(b[4] for b in used)


# ---------------------------------------------------------------- the consensus rules, one test a rule ----------------------------------------
def pileup_of(templates, used, columns=(), slots=()):
    """a pileup dict in which every column holds `used` copies of the template's own base, then the given (m, j, counts) rows"""
    M = len(templates)
    col_off = np.concatenate([[0], np.cumsum([len(t) for t in templates])]).astype(np.uint64)
    total = int(col_off[M])
    p = {"n_templates": M, "col_off": col_off, "columns": np.zeros((total, 6), np.uint32), "slots": np.zeros((total + M, 5), np.uint32),
         "score_sum": np.zeros(M, np.int64), "used": np.array(used, np.uint64)}
    for name in ("partial", "long_", "weak"):
        p[name] = np.zeros(M, np.uint64)
    for m, t in enumerate(templates):
        for j, c in enumerate(t):
            p["columns"][int(col_off[m]) + j, code(c)] = used[m]
    for m, j, counts in columns:
        p["columns"][int(col_off[m]) + j] = counts
    for m, j, counts in slots:
        p["slots"][int(col_off[m]) + m + j] = counts
    return p


def vote(templates, used, columns=(), slots=()):
    r = capi.monomer_consensus(pileup_of(templates, used, columns, slots), templates)
    assert r["changed"] == [a != b for a, b in zip(r["templates"], templates)] and r["rounds"] == 0 and r["names"] is None
    return r["templates"]


def test_consensus_tie_goes_to_the_templates_own_base():
    assert vote(["ACGT"], [10], columns=[(0, 2, [5, 0, 5, 0, 0, 0])]) == ["ACGT"]
    assert vote(["ACgT"], [10], columns=[(0, 2, [5, 0, 5, 0, 0, 0])]) == ["ACGT"]        # case-folded, written in upper case
    assert vote(["ACGT"], [10], columns=[(0, 2, [6, 0, 4, 0, 0, 0])]) == ["ACAT"]
    assert vote(["ACNT"], [10], columns=[(0, 2, [0, 0, 0, 0, 10, 0])]) == ["ACNT"]       # mx = 0: the character stays as it is
    assert vote(["ACnT"], [10], columns=[(0, 2, [0, 0, 0, 0, 6, 4])]) == ["ACnT"]


def test_consensus_tie_goes_to_acgt_order():
    assert vote(["ACGT"], [10], columns=[(0, 0, [0, 0, 5, 5, 0, 0])]) == ["GCGT"]
    assert vote(["ACGT"], [10], columns=[(0, 3, [3, 3, 3, 1, 0, 0])]) == ["ACGA"]
    assert vote(["ACNT"], [10], columns=[(0, 2, [0, 4, 0, 4, 2, 0])]) == ["ACCT"]


def test_consensus_drops_a_column_at_a_strict_majority_only():
    assert vote(["ACGT"], [10], columns=[(0, 1, [0, 5, 0, 0, 0, 5])]) == ["ACGT"]
    assert vote(["ACGT"], [10], columns=[(0, 1, [0, 4, 0, 0, 0, 6])]) == ["AGT"]
    assert vote(["ACGT"], [11], columns=[(0, 1, [0, 5, 0, 0, 0, 6])]) == ["AGT"]


def test_consensus_takes_one_base_a_slot_a_round():
    assert vote(["ACGT"], [10], slots=[(0, 2, [0, 0, 0, 6, 0])]) == ["ACTGT"]
    assert vote(["ACGT"], [10], slots=[(0, 2, [0, 0, 0, 5, 0])]) == ["ACGT"]              # half is no majority
    assert vote(["ACGT"], [10], slots=[(0, 0, [3, 3, 0, 0, 0]), (0, 4, [0, 0, 2, 2, 2])]) == ["AACGTG"]   # both ends, ties to ACGT order
    assert vote(["ACGT"], [10], slots=[(0, 1, [0, 0, 0, 0, 9])]) == ["ACGT"]              # nothing of ACGT recorded
    assert vote(["ACGT"], [10], slots=[(0, 1, [0, 1, 0, 0, 9])]) == ["ACCGT"]


def test_consensus_leaves_a_template_without_blocks():
    assert vote(["ACGT", "TTTT"], [0, 4], columns=[(0, 0, [0, 0, 0, 0, 0, 0])], slots=[(0, 1, [0, 9, 0, 0, 0])]) == ["ACGT", "TTTT"]


def test_consensus_leaves_a_template_whose_result_is_empty():
    assert vote(["AC", "G"], [10, 10], columns=[(0, 0, [0, 0, 0, 0, 0, 10]), (0, 1, [0, 0, 0, 0, 0, 10]), (1, 0, [0, 0, 0, 10, 0, 0])]) == ["AC", "T"]


def test_consensus_leaves_a_template_whose_result_has_1025_bases():
    t = "ACGT" * 256
    assert vote([t], [10], slots=[(0, 7, [9, 0, 0, 0, 0])]) == [t]
    assert vote([t], [10], slots=[(0, 7, [9, 0, 0, 0, 0])], columns=[(0, 100, [0, 0, 0, 0, 0, 10])]) == [t[:7] + "A" + t[7:100] + t[101:]]   # 1 024: taken


# ---------------------------------------------------------------- refinement: the runs of the prototype --------------------------------------
@pytest.fixture(scope="module")
def long_arrays():
    seqs = synth.hor_sequences(5, 40000, 2)
    assert synth.hor_monomers(5) == synth.hor_monomers(5) and len(seqs) == 2
    return seqs


def test_recovery_from_mutated_templates(long_arrays):
    truth = synth.hor_monomers(5)
    rng = random.Random(99)
    mutated = ["".join(synth._mut_track(rng, list(t), 0.05)[0]) for t in truth]
    assert all(a != b for a, b in zip(mutated, truth))
    r = capi.monomer_templates_refine_host(long_arrays, mutated, max_rounds=6, chunk=0)
    assert r["templates"] == truth and r["rounds"] == 2 and r["converged"] and r["changed"] == [True] * 12
    assert [q["changed"] for q in r["round"]] == [12, 0] and r["round"][1]["blocks"] == 466
    for kw in (dict(chunk=0), dict(chunk=4096, overlap=512)):
        dec = capi.monomer_decompose_host(long_arrays, truth, **kw)
        pile = capi.monomer_pileup_host(long_arrays, truth, dec, **kw)
        assert dec["n_blocks"] == 466 and pile["used"].tolist() == [40, 40, 40, 40] + [38] * 8
        assert capi.monomer_consensus(pile, truth)["changed"] == [False] * 12


def test_low_depth_changes_a_true_template(hor):
    """eight copies that share ancestral mutations outvote the truth: the documentation says so"""
    seqs, truth = hor
    r = capi.monomer_templates_refine_host(seqs, truth, max_rounds=4, chunk=0)
    assert r["rounds"] == 2 and r["converged"] and [q["changed"] for q in r["round"]] == [2, 0] and [q["blocks"] for q in r["round"]][0] == 129
    assert r["changed"] == [False] * 10 + [True, True]
    one = capi.monomer_templates_refine_host(seqs, truth, max_rounds=1, chunk=0)   # the round's vote is returned, and nobody has seen it hold
    assert one["templates"] == r["templates"] and one["rounds"] == 1 and not one["converged"] and one["round"] == r["round"][:1]
    dec = capi.monomer_decompose_host(seqs, truth, chunk=0)
    used = capi.monomer_pileup_host(seqs, truth, dec, chunk=0)["used"].tolist()
    assert used[10:] == [8, 8] and all(u in (10, 11) for u in used[:10])


# ---------------------------------------------------------------- seeds ------------------------------------------------------------------------
def test_seed_templates_and_their_refusals():
    seq = "ACGTTGCAAC" * 3
    r = capi.monomer_seed_templates([seq, "TTTT"], 4, 3, 2)
    assert r["templates"] == ["GTTG", "CAAC", "ACGT"] and r["names"] == ["seed1", "seed2", "seed3"] and r["changed"] == [False] * 3 and r["rounds"] == 0
    assert capi.monomer_seed_templates([seq], 30)["templates"] == [seq]
    assert capi.monomer_seed_templates(["NNNa"], 2, 1, 2)["templates"] == ["Na"]
    capi.monomer_seed_templates(["A" * 8192], 1024, 8)
    capi.monomer_seed_templates(["A" * 8192], 1024, 4, strands=2)
    bad = [("period", ([seq], 0)), ("period", ([seq], 1025)), ("count", ([seq], 4, 0)), ("count", (["A" * 9000], 1024, 9)), ("count", (["A" * 9000], 1024, 5, 0, 2)),
           ("start", ([seq], 4, 8)), ("start", ([seq], 4, 1, 27)), ("start", ([seq], 4, 1, 2 ** 40)), ("start", (["ACNNNNGT"], 2, 3, 0)), ("start", (["ACGT-*"], 2, 1, 4)),
           ("sequences", ([], 4)), ("strands", ([seq], 4, 1, 0, 3))]
    for word, args in bad:
        with pytest.raises(capi.ClError) as e:
            capi.monomer_seed_templates(*args)
        assert e.value.code == -1 and word in str(e.value), (args[1:], str(e.value))
    with pytest.raises(capi.ClError) as e:   # the length is checked, the bases behind it are never read
        capi.monomer_seed_templates(["ACGT"], 4, 2, 0, _lengths=[7])
    assert "start" in str(e.value)


@pytest.mark.parametrize("count", [1, 12])
def test_seeds_reach_a_fixed_point(long_arrays, count):
    seeds = capi.monomer_seed_templates(long_arrays, 171, count)["templates"]
    assert seeds == [long_arrays[0][k * 171:(k + 1) * 171] for k in range(count)]
    r = capi.monomer_templates_refine_host(long_arrays, seeds, max_rounds=8, chunk=0)
    assert r["converged"] and r["rounds"] <= 8 and r["round"][-1]["changed"] == 0 and len(r["templates"]) == count
    total = []
    for t in (seeds, r["templates"]):
        dec = capi.monomer_decompose_host(long_arrays, t, chunk=0)
        total.append(int(capi.monomer_pileup_host(long_arrays, t, dec, chunk=0)["score_sum"].sum()))
    assert total[1] >= total[0]
    if count == 1:   # a fixed point is one
        again = capi.monomer_templates_refine_host(long_arrays, r["templates"], max_rounds=3, chunk=0)
        assert again["rounds"] == 1 and again["converged"] and again["changed"] == [False]


# ---------------------------------------------------------------- the text --------------------------------------------------------------------
def pileup_rows(p, names, templates):
    rows = [PILEUP_HEADER]
    for m, t in enumerate(templates):
        c0 = int(p["col_off"][m])
        for j in range(len(t) + 1):
            col = p["columns"][c0 + j].tolist() if j < len(t) else [0] * 6
            rows.append("\t".join([names[m], str(j), t[j] if j < len(t) else "."] + [str(v) for v in col + p["slots"][c0 + m + j].tolist()]) + "\n")
    return "".join(rows).encode()


def test_text_writers():
    seq, templates = random_case(7, n_templates=3, length=300)
    templates[1] = templates[1].lower() + "N"
    dec = capi.monomer_decompose_host([seq], templates, chunk=0, strands=2)
    p = capi.monomer_pileup_host([seq], templates, dec, chunk=0, strands=2)
    names = ["m0", "second one", "m/2"]
    text = capi.monomer_pileup_tsv(p, names, templates)
    assert text == pileup_rows(p, names, templates) and text.count(b"\n") == 1 + sum(len(t) + 1 for t in templates) and p["slots"].sum() > 0
    hand = capi.monomer_pileup_host(["ACCGT"], ["ACGT"], dec_of([(0, 0, 5, 0, 3, 0)], 1))
    assert capi.monomer_pileup_tsv(hand, ["t"], ["ACGT"]).decode() == PILEUP_HEADER + (
        "t\t0\tA\t1\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n" "t\t1\tC\t0\t1\t0\t0\t0\t0\t0\t1\t0\t0\t0\n" "t\t2\tG\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0\t0\n"
        "t\t3\tT\t0\t0\t0\t1\t0\t0\t0\t0\t0\t0\t0\n" "t\t4\t.\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\n")
    assert capi.monomer_templates_fasta(names, templates) == "".join(">%s\n%s\n" % (n, t) for n, t in zip(names, templates)).encode()
    assert capi.monomer_templates_fasta(["seed1"], ["acgtN"]) == b">seed1\nacgtN\n"
    for thunk, word in ((lambda: capi.monomer_pileup_tsv(p, names[:2], templates[:2]), "pileup"), (lambda: capi.monomer_pileup_tsv(p, names, [t + "A" for t in templates]), "pileup"),
                        (lambda: capi.monomer_templates_fasta(["a"], [""]), "templates"), (lambda: capi.monomer_templates_fasta([], []), "templates"),
                        (lambda: capi.monomer_consensus(p, templates[:2]), "pileup"), (lambda: capi.monomer_consensus(p, ["A" * 1025] + templates[1:]), "templates")):
        with pytest.raises(capi.ClError) as e:
            thunk()
        assert e.value.code == -1 and word in str(e.value), str(e.value)


# ---------------------------------------------------------------- refused arguments, the ABI ----------------------------------------------------
def test_invalid_arguments():
    seqs, templates = ["ACGTACGTACGT", "ACGT"], ["ACGT", "TTG"]
    dec = capi.monomer_decompose_host(seqs, templates)
    capi.monomer_pileup_host(seqs, templates, dec)
    bad = [("match", dict(match=0)), ("mismatch", dict(mismatch=1)), ("insertion", dict(insertion=-65)), ("deletion", dict(deletion=0)), ("chunk", dict(chunk=63)),
           ("overlap", dict(overlap=2 ** 20 + 1)), ("strands", dict(strands=3))]
    for word, change in bad:
        for thunk in (lambda: capi.monomer_pileup_host(seqs, templates, dec, **change), lambda: capi.monomer_templates_refine_host(seqs, templates, **change)):
            with pytest.raises(capi.ClError) as e:
                thunk()
            assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    for templates_bad in ([], [""], ["A" * 1025], ["A" * 1024] * 9):
        for thunk in (lambda: capi.monomer_pileup_host(seqs, templates_bad, dec), lambda: capi.monomer_templates_refine_host(seqs, templates_bad)):
            with pytest.raises(capi.ClError) as e:
                thunk()
            assert e.value.code == -1 and "templates" in str(e.value)
    for share in (1001, 2 ** 32 - 1):
        for thunk in (lambda: capi.monomer_pileup_host(seqs, templates, dec, share), lambda: capi.monomer_templates_refine_host(seqs, templates, 2, share)):
            with pytest.raises(capi.ClError) as e:
                thunk()
            assert e.value.code == -1 and "least_share" in str(e.value)
    for rounds in (0, 65):
        with pytest.raises(capi.ClError) as e:
            capi.monomer_templates_refine_host(seqs, templates, rounds)
        assert e.value.code == -1 and "max_rounds" in str(e.value)
    capi.monomer_templates_refine_host(seqs, templates, 64, 1000)
    # a decomposition that does not fit the sequences or the templates is refused, not read
    for block in ((2, 0, 4, 0, 4, 0), (0, 0, 4, 2, 4, 0), (0, 0, 13, 0, 4, 0), (1, 0, 5, 0, 4, 0), (0, 5, 4, 0, 4, 0), (0, 2 ** 32 - 1, 2 ** 32 - 1, 0, 4, 0)):
        with pytest.raises(capi.ClError) as e:
            capi.monomer_pileup_host(seqs, templates, dec_of([(0, 0, 4, 0, 4, 0), block], 2))
        assert e.value.code == -1 and "dec" in str(e.value) and "block 1" in str(e.value), (block, str(e.value))
    capi.monomer_pileup_host(seqs, templates, dec_of([(0, 0, 4, 3, 4, 0)], 2), strands=2)   # monomer 3 exists with both strands
    for lens in ([2 ** 29, 2 ** 29], [2 ** 64 - 1, 2]):   # the lengths are checked before a base is read
        with pytest.raises(capi.ClError) as e:
            capi.monomer_pileup_host(seqs, templates, dec, _lengths=lens)
        assert e.value.code == -1 and "lengths" in str(e.value)
    empty = capi.monomer_pileup_host([], templates, dec_of([], 0))
    assert empty["used"].tolist() == [0, 0] and not empty["columns"].any() and empty["columns"].shape == (7, 6) and empty["slots"].shape == (9, 5)


def test_abi():
    lib = capi.load_library()
    new = ["cl_monomer_pileup_host", "cl_monomer_pileup_compute", "cl_monomer_pileup_free", "cl_monomer_consensus", "cl_monomer_templates_refine_host",
           "cl_monomer_templates_refine_compute", "cl_monomer_templates_free", "cl_monomer_seed_templates", "cl_monomer_pileup_tsv", "cl_monomer_templates_fasta"]
    for sym in new:
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    lib.cl_abi_version.restype = C.c_int
    assert lib.cl_abi_version() == 22
    # the header's layouts by hand (LP64): {u64, 8 pointers, 2 floats}, {3 x u64, 4 floats}, {u64, 4 pointers, 2 x 4 bytes, pointer}
    sizes_by_hand = [80, 40, 56]
    assert [C.sizeof(capi.MonomerPileupC), C.sizeof(capi.MonomerRound), C.sizeof(capi.MonomerTemplatesC)] == sizes_by_hand
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is not None:
        src = ('#include <stdio.h>\n#include "centrolign_amd.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(cl_monomer_pileup), sizeof(cl_monomer_round), '
               'sizeof(cl_monomer_templates), sizeof(cl_monomers_params), sizeof(cl_monomer_decomposition)); return 0; }\n')
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "s.c"), "w") as f:
                f.write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
            sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()]
        assert sizes == sizes_by_hand + [28, 48]


# ---------------------------------------------------------------- the command line ------------------------------------------------------------
def run_cli(args, **kw):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=60, **kw)


@pytest.fixture()
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGAACGTACGTACGTACGTACGT\n")
    return p


@pytest.fixture()
def templates_fa(tmp_path):
    p = tmp_path / "templates.fa"
    p.write_text(">m0\nACGTACG\n>m1\nTTGCA\n")
    return p


def test_cli_refusals(tmp_path, fasta, templates_fa):
    """each is one "error:" line and status 1 with nothing on standard output and no file made, before the FASTA is read or a device opened"""
    out, new, pile, old, other = tmp_path / "monomers.tsv", tmp_path / "new.fa", tmp_path / "pileup.tsv", tmp_path / "old.tsv", tmp_path / "other.tsv"
    old.write_text("keep me\n")
    t = ["--monomers-templates", templates_fa]
    d = ["--monomers", out] + t
    seeded = ["--monomers", out, "--monomers-seed-period", 7]
    cases = {
        "rounds alone": ["--monomers-rounds", 2, fasta],
        "write-templates alone": ["--monomers-write-templates", new, fasta],
        "pileup alone": ["--monomers-pileup", pile, fasta],
        "least-share alone": ["--monomers-least-share", 5, fasta],
        "seed-period alone": ["--monomers-seed-period", 7, fasta],
        "seed-count alone": ["--monomers-seed-count", 2, fasta],
        "seed-start alone": ["--monomers-seed-start", 2, fasta],
        "neither templates nor seeds": ["--monomers", out, "--monomers-rounds", 2, fasta],
        "templates and seeds": d + ["--monomers-seed-period", 7, fasta],
        "seed-count without seed-period": d + ["--monomers-seed-count", 2, fasta],
        "seed-start without seed-period": d + ["--monomers-seed-start", 2, fasta],
        "write-templates without rounds or seeds": d + ["--monomers-write-templates", new, fasta],
        "an existing templates file": d + ["--monomers-rounds", 2, "--monomers-write-templates", old, fasta],
        "an existing pileup file": d + ["--monomers-pileup", old, fasta],
        "the pileup in the file of --monomers": d + ["--monomers-pileup", out, fasta],
        "the pileup in the summary's file": d + ["--monomers-summary", other, "--monomers-pileup", other, fasta],
        "the pileup in the templates' file": d + ["--monomers-pileup", templates_fa, fasta],
        "the new templates in the given templates' file": d + ["--monomers-rounds", 2, "--monomers-write-templates", templates_fa, fasta],
        "the new templates in the file of --monomers": d + ["--monomers-rounds", 2, "--monomers-write-templates", out, fasta],
        "one file for templates and pileup": d + ["--monomers-rounds", 2, "--monomers-write-templates", new, "--monomers-pileup", new, fasta],
        "the pileup in the file of --periods": d + ["--monomers-pileup", pile, "--periods", pile, fasta],
        "the pileup in the file of --dotplot": d + ["--monomers-pileup", pile, "--dotplot", pile, fasta],
        "the new templates in the file of --pair-stats": seeded + ["--monomers-write-templates", new, "--pair-stats", new, fasta],
        "the new templates in the file of --msa-out": seeded + ["--monomers-write-templates", new, "--msa-out", new, fasta],
        "an empty pileup file name": d + ["--monomers-pileup", "", fasta],
        "too many seed bases": ["--monomers", out, "--monomers-seed-period", 1024, "--monomers-seed-count", 9, fasta],
        "too many seed bases on both strands": ["--monomers", out, "--monomers-seed-period", 1024, "--monomers-seed-count", 5, "--monomers-strands", "both", fasta],
        "only with --periods": d + ["--monomers-rounds", 2, "--monomers-only", "--periods", other, fasta],
        "with --graph": seeded + ["--graph", other, "--compare-to", other, "--pair-agreement", tmp_path / "agree.tsv"],
    }
    numbers = {"--monomers-rounds": (1, 64, d), "--monomers-least-share": (0, 1000, d), "--monomers-seed-period": (1, 1024, ["--monomers", out]),
               "--monomers-seed-count": (1, None, seeded), "--monomers-seed-start": (0, 2 ** 30 - 1, seeded)}
    for opt, (least, most, base) in numbers.items():
        for name, value in (("not a number", "x"), ("a fraction", "2.5"), ("empty", ""), ("negative", -1), ("below the limit", least - 1)) + (
                (("above the limit", most + 1),) if most else ()):
            cases["%s %s" % (opt, name)] = base + [opt, value, fasta]
    assert len(cases) >= 55
    for name, args in cases.items():
        r = run_cli(args)
        err = r.stderr.decode().splitlines()
        assert r.returncode == 1 and r.stdout == b"", (name, r.returncode, r.stderr)
        assert len(err) == 1 and err[0].startswith("error: ") and "GPU" not in err[0], (name, err)
        for made in (out, new, pile, other):
            assert not made.exists(), (name, made)
        assert old.read_text() == "keep me\n" and templates_fa.read_text().startswith(">m0\n"), name
    # they come before the FASTA is read, and the extreme values pass: the run then ends at the FASTA that is not there
    r = run_cli(d + ["--monomers-rounds", 65, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"--monomers-rounds" in r.stderr and b"missing.fa" not in r.stderr
    for pick in (0, 1):
        args = ["--monomers", out, "--monomers-only", "--monomers-write-templates", new, "--monomers-pileup", pile, "--monomers-rounds", (1, 64)[pick],
                "--monomers-least-share", (0, 1000)[pick], "--monomers-seed-period", (1, 1024)[pick], "--monomers-seed-count", (1, 8)[pick],
                "--monomers-seed-start", (0, 2 ** 30 - 1)[pick]]
        r = run_cli(args + [tmp_path / "missing.fa"])
        assert r.returncode == 1 and b"missing.fa" in r.stderr and not out.exists() and not new.exists() and not pile.exists(), r.stderr
    # the seed range is checked once the FASTA is read, still without a device
    for args in (["--monomers-seed-period", 29], ["--monomers-seed-period", 7, "--monomers-seed-count", 5], ["--monomers-seed-period", 7, "--monomers-seed-start", 22]):
        r = run_cli(["--monomers", out, "--monomers-only"] + args + [fasta])
        err = [line for line in r.stderr.decode().splitlines() if line.startswith("error: ")]   # (behind the progress lines of reading the input)
        assert r.returncode == 1 and r.stdout == b"" and len(err) == 1 and err[0].startswith("error: --monomers-seed-period") and b"GPU" not in r.stderr, r.stderr
        assert not out.exists()


def test_cli_help_generate_config_and_abbreviations(tmp_path, templates_fa):
    text = run_cli(["-h"]).stderr.decode()
    for opt in ("--monomers-rounds INT", "--monomers-write-templates FASTA", "--monomers-pileup FILE", "--monomers-least-share INT", "--monomers-seed-period INT",
                "--monomers-seed-count INT", "--monomers-seed-start INT"):
        assert opt in text, opt
    plain = run_cli(["-G"])
    with_options = run_cli(["-G", "--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, "--monomers-rounds", 3, "--monomers-write-templates",
                            tmp_path / "new.fa", "--monomers-pileup", tmp_path / "pileup.tsv", "--monomers-least-share", 500])
    seeded = run_cli(["-G", "--monomers", tmp_path / "monomers.tsv", "--monomers-seed-period", 7, "--monomers-seed-count", 2, "--monomers-seed-start", 1])
    assert plain.returncode == 0 and plain.stdout and plain.stdout == with_options.stdout == seeded.stdout and b"monomers" not in plain.stdout
    assert not list(tmp_path.glob("*.tsv")) and not (tmp_path / "new.fa").exists()
    # every abbreviation of the options that were there keeps its meaning
    old = tmp_path / "old.tsv"
    old.write_text("keep me\n")
    for short, message in (("--monomers-t", b"Monomer decomposition file already exists"), ("--monomers-te", b"Monomer decomposition file already exists")):
        r = run_cli(["--monomers", old, short, templates_fa, tmp_path / "missing.fa"])
        assert r.returncode == 1 and message in r.stderr, (short, r.stderr)
    for short, word in (("--monomers-c", b"--monomers-chunk"), ("--monomers-i", b"--monomers-insertion"), ("--monomers-d", b"--monomers-deletion"), ("--monomers-ma", b"--monomers-match"),
                        ("--monomers-mi", b"--monomers-mismatch"), ("--monomers-ov", b"--monomers-overlap"), ("--monomers-st", b"--monomers-strands")):
        r = run_cli(["--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, short, "x", tmp_path / "missing.fa"])
        assert r.returncode == 1 and word in r.stderr and b"missing.fa" not in r.stderr, (short, r.stderr)
    r = run_cli(["--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, "--monomers-su", old, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"Monomer summary file already exists" in r.stderr
    r = run_cli(["--monomers-on", tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"--monomers-only needs --monomers" in r.stderr
