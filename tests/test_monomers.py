"""Monomer decomposition (cl_monomer_decompose_host, the two TSV writers, the CLI's --monomers options), without a GPU: the host definition against
two restatements that share no code with the library and little with each other (`problem_tuples`: the definition line by line in Python
tuples, the deletion maximum over every k; `problem_rows`: one numpy row at a time for the long cases), hand-made cases for every tie rule, the
higher-order-repeat arrays, chunks against the whole, both strands, the text, every refused argument, the ABI, and every refusal of the command
line, which comes before a device is opened.  tests/test_gpu_monomers.py holds the device path against the same restatements."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
SCORE_SETS = [(1, -1, -1, -1), (2, -3, -2, -2), (1, -4, -1, -6), (5, -1, -15, -1)]
HOR_CHUNKINGS = [(2048, 512), (1024, 256), (512, 400)]
TSV_HEADER = "sample\tstart\tend\tmonomer\tstrand\tscore\tshare\tpartial\n"
SUMMARY_HEADER = "sample\tmonomer\tstrand\tblocks\tbases\tscore\n"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}


def revcomp(t):
    return "".join(_COMP.get(c, c) for c in reversed(t))


def same_base(a, b):
    a, b = a.upper(), b.upper()
    return a in "ACGT" and a == b


def blocks_from(n, E, rec, H, templates):
    """the closing cell and the walk back: [(start, end, m, score, flags)] ascending, in the problem's own coordinates"""
    close = None
    for m, B in enumerate(templates):
        for j in range(1, len(B) + 1):
            key = (H[m][j][0], H[m][j][1], -m, j)   # larger score, larger start, smaller m, larger j
            if close is None or key > close[0]:
                close = (key, m, j)
    (score, start, _, _), m, j = close
    out = [(max(start, 0), n, m, score - E[max(start, 0)], (1 if start == -1 else 0) | (2 if j < len(templates[m]) else 0))]
    i = out[0][0]
    while i > 0:
        score, start, m = rec[i]
        out.append((max(start, 0), i, m, score - E[max(start, 0)], 1 if start == -1 else 0))
        i = max(start, 0)
    return out[::-1]


def problem_tuples(S, templates, scores):
    """the definition, line by line"""
    match, mismatch, ins, dele = scores
    n = len(S)
    if n == 0:
        return []
    H = [[(0, 0)] + [(0, -1)] * len(B) for B in templates]
    E, rec = [0], [None]
    for i in range(1, n + 1):
        Ds = []
        for m, B in enumerate(templates):
            T = [None] * (len(B) + 1)
            for j in range(1, len(B) + 1):
                s = match if same_base(S[i - 1], B[j - 1]) else mismatch
                T[j] = max((H[m][j - 1][0] + s, H[m][j - 1][1]), (H[m][j][0] + ins, H[m][j][1]))
            Ds.append([None] + [max((T[k][0] + (j - k) * dele, T[k][1]) for k in range(1, j + 1)) for j in range(1, len(B) + 1)])
        best = max(range(len(templates)), key=lambda m: (Ds[m][-1], -m))
        rec.append((Ds[best][-1][0], Ds[best][-1][1], best))
        E.append(Ds[best][-1][0])
        H = [[(E[i], i)] + [max(D[j], (E[i] + j * dele, i)) for j in range(1, len(D))] for D in Ds]
    return blocks_from(n, E, rec, H, templates)


_CODE = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def problem_rows(S, templates, scores):
    """the same with one numpy row per sequence base: a value is score * 2^32 + start + 1 in an int64, templates padded to one length"""
    match, mismatch, ins, dele = scores
    n, M, BIG, NEG = len(S), len(templates), 1 << 32, -(1 << 62)
    if n == 0:
        return []
    lens = np.array([len(B) for B in templates])
    width = int(lens.max())
    j = np.arange(1, width + 1, dtype=np.int64)
    valid = j[None, :] <= lens[:, None]
    tb = np.full((M, width), 5, np.int64)
    for m, B in enumerate(templates):
        c = _CODE[np.frombuffer(B.encode(), np.uint8)]
        tb[m, :len(B)] = np.where(c > 3, 5, c)
    sc = _CODE[np.frombuffer(S.encode(), np.uint8)]
    H = np.where(valid, 0, NEG).astype(np.int64)
    E, rec = [0], [None]
    jd = j * dele * BIG
    for i in range(1, n + 1):
        diag = np.concatenate([np.full((M, 1), E[i - 1] * BIG + i, np.int64), H[:, :-1]], axis=1)
        T = np.maximum(diag + np.where(tb == sc[i - 1], match, mismatch) * BIG, H + ins * BIG)
        D = np.maximum.accumulate(T - jd, axis=1) + jd
        last = D[np.arange(M), lens - 1]
        m = int(np.argmax(last))   # the first of the largest: the smallest m
        score, start1 = divmod(int(last[m]), BIG)
        rec.append((score, start1 - 1, m))
        E.append(score)
        H = np.where(valid, np.maximum(D, (score + j * dele) * BIG + i + 1), NEG)
    cells = [[None] + [(lambda v: (v[0], v[1] - 1))(divmod(int(H[m, k]), BIG)) for k in range(len(B))] for m, B in enumerate(templates)]
    return blocks_from(n, E, rec, cells, templates)


def restated(seqs, templates, scores=(1, -1, -1, -1), chunk=0, overlap=0, strands=1, problem=problem_tuples):
    """(blocks as capi.MONOMER_BLOCK, n_problems) by the definition's chunk rule"""
    both = list(templates) + ([revcomp(t) for t in templates] if strands == 2 else [])
    out, n_problems = [], 0
    for s, seq in enumerate(seqs):
        L = len(seq)
        ranges = [(0, L, 0, L + 1)] if chunk == 0 else [(max(0, c * chunk - overlap), min(L, (c + 1) * chunk + overlap), c * chunk, (c + 1) * chunk)
                                                       for c in range((L + chunk - 1) // chunk)]
        n_problems += len(ranges)
        for lo, hi, keep_lo, keep_hi in ranges:
            for start, end, m, score, flags in problem(seq[lo:hi], both, scores):
                if keep_lo <= lo + start < keep_hi:
                    out.append((s, lo + start, lo + end, m, score, flags))
    return np.array(out, capi.MONOMER_BLOCK), n_problems


def same_blocks(got, want_blocks, want_problems=None):
    assert got["n_blocks"] == len(want_blocks) == len(got["blocks"])
    if not np.array_equal(got["blocks"], want_blocks):
        k = int(np.nonzero(got["blocks"] != want_blocks)[0][0])
        raise AssertionError("block %d: got %s, want %s" % (k, got["blocks"][k], want_blocks[k]))
    if want_problems is not None:
        assert got["n_problems"] == want_problems
    seq_off = np.searchsorted(want_blocks["sequence"], np.arange(got["n_seq"] + 1))
    assert np.array_equal(got["seq_off"], seq_off)


def params(scores=(1, -1, -1, -1), **kw):
    return dict(zip(("match", "mismatch", "insertion", "deletion"), scores), **kw)


def check_host(seqs, templates, scores=(1, -1, -1, -1), chunk=0, overlap=0, strands=1, problem=problem_tuples):
    want, n_problems = restated(seqs, templates, scores, chunk, overlap, strands, problem)
    got = capi.monomer_decompose_host(seqs, templates, **params(scores, chunk=chunk, overlap=overlap, strands=strands))
    same_blocks(got, want, n_problems)
    assert got["dp_ms"] == 0 and got["trace_ms"] == 0
    return want


def tsv_rows(blocks, names, tnames, tlens, match=1):
    M = len(tnames)
    rows = [TSV_HEADER]
    for b in blocks:
        m = int(b["monomer"]) % M
        rows.append("%s\t%d\t%d\t%s\t%s\t%d\t%s\t%s\n" % (names[b["sequence"]], b["start"], b["end"], tnames[m], "+" if b["monomer"] < M else "-", b["score"],
                                                        "%.9g" % (int(b["score"]) / (match * tlens[m])), (".", "L", "R", "LR")[b["flags"]]))
    return "".join(rows).encode()


def summary_rows(blocks, names, tnames):
    M = len(tnames)
    rows = [SUMMARY_HEADER]
    for s, name in enumerate(names):
        for m in range(M):
            for strand, mono in (("+", m), ("-", M + m)):
                sel = blocks[(blocks["sequence"] == s) & (blocks["monomer"] == mono)]
                if len(sel):
                    rows.append("%s\t%s\t%s\t%d\t%d\t%d\n" % (name, tnames[m], strand, len(sel), int((sel["end"].astype(np.int64) - sel["start"]).sum()),
                                                           int(sel["score"].astype(np.int64).sum())))
    return "".join(rows).encode()


# ---------------------------------------------------------------- the restatements agree with each other ----------------------------------------
def random_case(seed, n_templates=3, length=120):
    rng = np.random.default_rng(seed)
    templates = ["".join("ACGT"[x] for x in rng.integers(0, 4, int(rng.integers(1, 12)))) for _ in range(n_templates)]
    pool = templates + [revcomp(t) for t in templates]
    seq = ""
    while len(seq) < length:
        unit = list(pool[int(rng.integers(0, len(pool)))])
        for _ in range(int(rng.integers(0, 3))):
            at = int(rng.integers(0, len(unit) + 1))
            unit[at:at + 1] = [[], ["N"], ["a", "c"], ["T"]][int(rng.integers(0, 4))]
        seq += "".join(unit)
    return seq[:length], templates


@pytest.mark.parametrize("scores", SCORE_SETS)
def test_the_two_restatements_agree(scores):
    for seed in range(4):
        seq, templates = random_case(seed)
        assert problem_tuples(seq, templates, scores) == problem_rows(seq, templates, scores)


# ---------------------------------------------------------------- hand-made cases -------------------------------------------------------------
def test_one_base_template():
    want = check_host(["AAAA"], ["A"])
    assert want.tolist() == [(0, k, k + 1, 0, 1, 0) for k in range(4)]


def test_every_tie_rule():
    """"A" and "AA" on runs of A: a block of "AA" scores what two blocks of "A" do, so the larger start, the smallest m and the largest j all decide"""
    for seq in ("A", "AA", "AAA", "AAAAAAA", "AAACAAAA", "CAAAC"):
        for templates in (["A", "AA"], ["AA", "A"], ["AA", "A", "AA", "A"]):
            for scores in SCORE_SETS:
                check_host([seq], templates, scores)
    want = check_host(["AAAA"], ["A", "AA"])
    assert want["monomer"].tolist() == [0, 0, 0, 0] and want["score"].tolist() == [1, 1, 1, 1]   # the larger start wins over the longer template


def test_identical_templates():
    seq, templates = random_case(11)
    want = check_host([seq], [templates[0], templates[1], templates[0], templates[1]])
    assert set(want["monomer"].tolist()) <= {0, 1}


def test_short_sequences():
    templates = ["ACGTACG", "TTGCA"]
    for seq in ("", "A", "ACG", "GTAC", "ACGTAC", "N", "TTGCAACGTACG"):
        for scores in SCORE_SETS:
            check_host([seq], templates, scores)
    none = capi.monomer_decompose_host([""], templates, chunk=0)
    assert none["n_blocks"] == 0 and none["n_problems"] == 1 and none["seq_off"].tolist() == [0, 0]
    assert capi.monomer_decompose_host(["", ""], templates, chunk=64)["n_problems"] == 0
    nothing = capi.monomer_decompose_host([], templates)
    assert nothing["n_blocks"] == 0 and nothing["n_seq"] == 0 and nothing["seq_off"].tolist() == [0]
    one = check_host(["A"], templates)
    assert len(one) == 1 and one[0]["flags"] & 2   # a sequence shorter than a template: a partial block


def test_other_characters_and_case():
    templates = ["ACGTNACGT", "acgtTTTT", "RYACGT"]
    for seq in ("ACGTNACGTacgtttttRYACGT", "NNNNNNNN", "acgtnacgtACGTTTTTryacgt", "ACGT-ACGT*ACGT"):
        want = check_host([seq], templates)
        assert len(want)
    upper = check_host(["ACGTTACGTACGTTTTT"], ["ACGTTACGT", "ACGTTTTT"])
    lower = check_host(["acgttacgtacgttttt"], ["ACGTTACGT", "ACGTTTTT"])
    assert np.array_equal(upper, lower)
    # N matches nothing, not even N
    assert check_host(["ACGTNACGT"], ["ACGTNACGT"])["score"].sum() < 9 and check_host(["ACGTAACGT"], ["ACGTAACGT"])["score"].tolist() == [9]


def test_partial_blocks_at_both_ends():
    unit = "ACGGTCATTGCA"
    want = check_host([unit[7:] + unit * 3 + unit[:5]], [unit])
    assert want["flags"].tolist() == [1, 0, 0, 0, 2] and want["start"].tolist() == [0, 5, 17, 29, 41] and want["score"].tolist() == [5, 12, 12, 12, 5]
    assert check_host([unit[3:9]], [unit])["flags"].tolist() == [3]   # inside one template: partial on both sides


@pytest.mark.parametrize("scores", SCORE_SETS)
def test_score_sets(scores):
    for seed in (1, 2, 3):
        seq, templates = random_case(seed, n_templates=4, length=200)
        check_host([seq, seq[50:120]], templates, scores)
        check_host([seq, seq[50:120]], templates, scores, strands=2)
        check_host([seq], templates, scores, chunk=64, overlap=20)


def test_chunks_by_the_definition():
    seq, templates = random_case(5, length=400)
    for chunk, overlap in ((64, 0), (64, 1), (64, 70), (100, 33), (399, 5), (400, 0), (401, 0), (2 ** 20, 2 ** 20)):
        check_host([seq, "", seq[:65], seq[:64], seq[:63]], templates, chunk=chunk, overlap=overlap)


# ---------------------------------------------------------------- higher-order-repeat arrays --------------------------------------------------
@pytest.fixture(scope="module")
def hor():
    seqs = synth.hor_sequences(5, 6000, 3)
    assert [len(s) for s in seqs] == [5998, 10128, 5996]
    templates = synth.hor_monomers(5)
    assert len(templates) == 12 and synth.hor_sequences(5, 6000, 3) == seqs   # the same seed gives the same arrays with and without the templates drawn
    return seqs, templates


@pytest.fixture(scope="module")
def hor_whole(hor):
    """the unchunked blocks of the three arrays by the numpy restatement, computed once"""
    return restated(hor[0], hor[1], problem=problem_rows)


def test_hor_arrays(hor, hor_whole):
    seqs, templates = hor
    want, n_problems = hor_whole
    got = capi.monomer_decompose_host(seqs, templates, chunk=0)
    same_blocks(got, want, n_problems)
    assert np.diff(got["seq_off"]).tolist() == [35, 59, 35]
    for s in range(3):
        b = want[got["seq_off"][s]:got["seq_off"][s + 1]]
        assert b["monomer"].tolist() == [k % 12 for k in range(len(b))]   # the cyclic order from the first block on
        assert b["start"][0] == 0 and b["end"][-1] == len(seqs[s]) and np.array_equal(b["start"][1:], b["end"][:-1])   # the blocks tile the sequence
        # the last one is a partial-right block of monomer 10; the first begins inside monomer 0 (the arrays start at a mutated copy's first base)
        assert b["monomer"][-1] == 10 and b["flags"][-1] == 2 and not b["flags"][1:-1].any()
        assert (b["score"][:-1] > 100).all()


@pytest.mark.parametrize("chunk,overlap", HOR_CHUNKINGS)
def test_hor_chunks_equal_the_whole(hor, hor_whole, chunk, overlap):
    got = capi.monomer_decompose_host(hor[0], hor[1], chunk=chunk, overlap=overlap)
    same_blocks(got, hor_whole[0], sum((len(s) + chunk - 1) // chunk for s in hor[0]))


def test_the_seam_is_real(hor, hor_whole):
    """with an overlap of one template length the blocks at a seam may differ: the documentation recommends two"""
    got = capi.monomer_decompose_host(hor[0], hor[1], chunk=1024, overlap=171)
    whole = set(map(tuple, hor_whole[0].tolist()))
    differing = [b for b in got["blocks"].tolist() if tuple(b) not in whole]
    assert 1 <= len(differing) <= 4 and all(b[0] == 1 for b in differing)


def test_the_defaults_equal_the_whole():
    """several default chunks of one array: if this fails the defaults are wrong, not the test"""
    d = capi.monomers_params_default()
    assert d == dict(match=1, mismatch=-1, insertion=-1, deletion=-1, chunk=4096, overlap=512, strands=1)
    seq = synth.hor_sequences(23, 4 * d["chunk"], 1)[0]
    templates = synth.hor_monomers(23)
    assert len(seq) > 3 * d["chunk"]
    by_default = capi.monomer_decompose_host([seq], templates)
    whole = capi.monomer_decompose_host([seq], templates, chunk=0)
    assert by_default["n_problems"] == (len(seq) + d["chunk"] - 1) // d["chunk"] >= 4 and whole["n_problems"] == 1
    same_blocks(by_default, whole["blocks"])


def test_strands(hor):
    seq, templates = hor[0][0][:3000], hor[1]
    flipped = seq[:1000] + revcomp(seq[1000:2000]) + seq[2000:]
    both = capi.monomer_decompose_host([flipped], templates, chunk=0, strands=2)["blocks"]
    inside = both[(both["start"] >= 1100) & (both["end"] <= 1900)]
    outside = both[(both["end"] <= 900) | (both["start"] >= 2100)]
    assert len(inside) >= 4 and (inside["monomer"] >= 12).all() and len(outside) >= 8 and (outside["monomer"] < 12).all()
    assert (inside["score"] > 100).all()
    forward = capi.monomer_decompose_host([flipped], templates, chunk=0, strands=1)["blocks"]
    inside = forward[(forward["start"] >= 1100) & (forward["end"] <= 1900)]
    assert (forward["monomer"] < 12).all() and len(inside) and (inside["score"] < 0.5 * 171).all()   # low share without the other strand
    want, _ = restated([flipped[800:1400]], templates, strands=2, problem=problem_rows)
    same_blocks(capi.monomer_decompose_host([flipped[800:1400]], templates, chunk=0, strands=2), want)


# ---------------------------------------------------------------- the text --------------------------------------------------------------------
def test_tsv():
    unit, other = "ACGGTCATTGCA", "TTGACCA"
    seqs = [unit[7:] + unit * 2 + revcomp(other) + other + unit[:5], "", revcomp(unit) + "NN"]
    names, tnames, tlens = ["chr1_a", "e", "c"], ["u", "o"], [len(unit), len(other)]
    for scores in ((1, -1, -1, -1), (2, -3, -2, -2)):
        dec = capi.monomer_decompose_host(seqs, [unit, other], **params(scores, chunk=0, strands=2))
        want, _ = restated(seqs, [unit, other], scores, strands=2)
        same_blocks(dec, want)
        text = capi.monomers_tsv(dec, names, tnames, tlens, **params(scores, strands=2))
        assert text == tsv_rows(want, names, tnames, tlens, scores[0]) and text.endswith(b"\n")
        summary = capi.monomers_summary_tsv(dec, names, tnames, tlens, **params(scores, strands=2))
        assert summary == summary_rows(want, names, tnames) and summary.endswith(b"\n")
    lines = capi.monomers_tsv(dec, names, tnames, tlens, match=2, strands=2).decode().splitlines()
    assert lines[0] == TSV_HEADER.rstrip("\n") and lines[1] == "chr1_a\t0\t5\tu\t+\t10\t0.416666667\tL"
    assert "chr1_a\t29\t36\to\t-\t14\t1\t." in lines and "chr1_a\t43\t48\tu\t+\t10\t0.416666667\tR" in lines and "c\t0\t14\tu\t-\t20\t0.833333333\t." in lines
    assert not any(line.startswith("e\t") for line in lines)
    assert b"chr1_a\tu\t+\t4\t" in summary and b"chr1_a\to\t-\t1\t7\t14\n" in summary and b"\nc\tu\t-\t" in summary
    empty = capi.monomer_decompose_host([""], [unit])
    assert capi.monomers_tsv(empty, ["e"], ["u"], [12]) == TSV_HEADER.encode() and capi.monomers_summary_tsv(empty, ["e"], ["u"], [12]) == SUMMARY_HEADER.encode()
    with pytest.raises(capi.ClError) as e:
        capi.monomers_tsv(dec, names, ["u"], [12], strands=1)   # blocks of templates the writer was not given
    assert e.value.code == -1 and "blocks" in str(e.value)


# ---------------------------------------------------------------- refused arguments, the ABI ----------------------------------------------------
def test_invalid_arguments():
    seqs, templates = ["ACGTACGTACGT"], ["ACGT"]
    capi.monomer_decompose_host(seqs, templates)
    bad = [("match", dict(match=0)), ("match", dict(match=-1)), ("match", dict(match=65)), ("mismatch", dict(mismatch=0)), ("mismatch", dict(mismatch=1)),
           ("mismatch", dict(mismatch=-65)), ("insertion", dict(insertion=0)), ("insertion", dict(insertion=-65)), ("deletion", dict(deletion=0)),
           ("deletion", dict(deletion=3)), ("deletion", dict(deletion=-65)), ("chunk", dict(chunk=1)), ("chunk", dict(chunk=63)), ("chunk", dict(chunk=2 ** 20 + 1)),
           ("overlap", dict(overlap=2 ** 20 + 1)), ("strands", dict(strands=0)), ("strands", dict(strands=3))]
    for word, change in bad:
        with pytest.raises(capi.ClError) as e:
            capi.monomer_decompose_host(seqs, templates, **change)
        assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    for templates_bad in ([], [""], ["ACGT", ""], ["A" * 1025], ["A" * 1024] * 9, ["A" * 1024] * 5 + ["C"]):
        with pytest.raises(capi.ClError) as e:
            capi.monomer_decompose_host(seqs, templates_bad, strands=2 if len(templates_bad) == 6 else 1)
        assert e.value.code == -1 and "templates" in str(e.value), (len(templates_bad), str(e.value))
    # the largest values of every argument are accepted
    capi.monomer_decompose_host(seqs, ["A" * 1024] * 8, match=64, mismatch=-64, insertion=-64, deletion=-64, chunk=2 ** 20, overlap=2 ** 20)
    capi.monomer_decompose_host(seqs, ["A" * 1024] * 4, strands=2, chunk=64, overlap=0)
    capi.monomer_decompose_host(seqs, ["A"] * 8192, chunk=0)


def test_too_much_text_is_refused():
    """the lengths are checked before a base is read: 2^30 bases in all, from buffers that are far shorter"""
    for lens in ([2 ** 29, 2 ** 29], [2 ** 30, 0], [2 ** 64 - 1, 2]):
        with pytest.raises(capi.ClError) as e:
            capi.monomer_decompose_host(["ACGT", "ACGT"], ["ACGT"], _lengths=lens)
        assert e.value.code == -1 and "lengths" in str(e.value)


def test_abi():
    lib = capi.load_library()
    new = ["cl_monomers_params_default", "cl_monomer_decompose_host", "cl_monomer_decompose_compute", "cl_monomers_tsv", "cl_monomers_summary_tsv",
           "cl_monomer_decomposition_free"]
    for sym in new:
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    lib.cl_abi_version.restype = C.c_int
    assert lib.cl_abi_version() == 22
    assert C.sizeof(capi.MonomerBlock) == 24 == capi.MONOMER_BLOCK.itemsize
    # the header's layouts by hand (LP64): 7 x 4 bytes, 6 x 4 bytes, {3 x u64, 2 pointers, 2 floats}
    assert [C.sizeof(capi.MonomersParams), C.sizeof(capi.MonomerBlock), C.sizeof(capi.MonomerDecompositionC)] == [28, 24, 48]
    # and the C compiler's own sizes from the header itself, where there is a compiler
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is not None:
        src = ('#include <stdio.h>\n#include "centrolign_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(cl_monomers_params), sizeof(cl_monomer_block), '
               'sizeof(cl_monomer_decomposition)); return 0; }\n')
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "s.c"), "w") as f:
                f.write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
            sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()]
        assert sizes == [28, 24, 48]


# ---------------------------------------------------------------- the command line ------------------------------------------------------------
def run_cli(args, **kw):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=60, **kw)


@pytest.fixture()
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGAACGTACGTACGTACGTACGT\n>c\nACGTACGAACGTACGTACGGACGTACGT\n")
    return p


@pytest.fixture()
def templates_fa(tmp_path):
    p = tmp_path / "templates.fa"
    p.write_text(">m0\nACGTACG\n>m1 the second\nTTGCA\nTTG\n")
    return p


NUMBERS = {"--monomers-match": (1, 64, 2), "--monomers-mismatch": (-64, -1, -2), "--monomers-insertion": (-64, -1, -2), "--monomers-deletion": (-64, -1, -2),
           "--monomers-chunk": (64, 2 ** 20, 100), "--monomers-overlap": (0, 2 ** 20, 30)}


def refusals(tmp_path, fasta, templates_fa):
    out, summary, old, other = tmp_path / "monomers.tsv", tmp_path / "summary.tsv", tmp_path / "old.tsv", tmp_path / "other.tsv"
    old.write_text("keep me\n")
    t = ["--monomers-templates", templates_fa]
    d = ["--monomers", out] + t
    files = {}
    for name, text in (("none.fa", ""), ("empty.fa", ">m0\n\n>m1\nACGT\n"), ("long.fa", ">m0\n" + "A" * 1025 + "\n"),
                       ("many.fa", "".join(">m%d\n%s\n" % (k, "ACGT" * 256) for k in range(9))), ("five.fa", "".join(">m%d\n%s\n" % (k, "ACGT" * 256) for k in range(5)))):
        files[name] = tmp_path / name
        files[name].write_text(text)
    cases = {
        "an existing file": ["--monomers", old] + t + [fasta],
        "an existing summary file": d + ["--monomers-summary", old, fasta],
        "one file for both": d + ["--monomers-summary", out, fasta],
        "the file of --pair-stats": d + ["--pair-stats", out, fasta],
        "the file of --tree-out": d + ["--infer-tree", "--tree-out", out, fasta],
        "the file of --msa-out": d + ["--msa-out", out, fasta],
        "the file of -s": d + ["-s", out, fasta],
        "the file of --dotplot": d + ["--dotplot", out, fasta],
        "the file of --periods": d + ["--periods", out, fasta],
        "the summary in the file of --column-stats": d + ["--monomers-summary", summary, "--column-stats", summary, fasta],
        "the summary in the file of --periods-hist": d + ["--monomers-summary", summary, "--periods", other, "--periods-hist", summary, fasta],
        "the templates' file": ["--monomers", templates_fa] + t + [fasta],
        "no templates": ["--monomers", out, fasta],
        "templates that are not there": ["--monomers", out, "--monomers-templates", tmp_path / "missing_templates.fa", fasta],
        "a templates file without a template": ["--monomers", out, "--monomers-templates", files["none.fa"], fasta],
        "an empty template": ["--monomers", out, "--monomers-templates", files["empty.fa"], fasta],
        "a template of 1025 bases": ["--monomers", out, "--monomers-templates", files["long.fa"], fasta],
        "9216 template bases": ["--monomers", out, "--monomers-templates", files["many.fa"], fasta],
        "5120 template bases on both strands": ["--monomers", out, "--monomers-templates", files["five.fa"], "--monomers-strands", "both", fasta],
        "strands word": d + ["--monomers-strands", "reverse", fasta],
        "chunk 63": d + ["--monomers-chunk", 63, fasta],
        "mismatch 0": d + ["--monomers-mismatch", 0, fasta],
        "mismatch 1": d + ["--monomers-mismatch", 1, fasta],
        "--monomers-templates alone": t + [fasta],
        "--monomers-summary alone": ["--monomers-summary", summary, fasta],
        "--monomers-strands alone": ["--monomers-strands", "both", fasta],
        "--monomers-only alone": ["--monomers-only", fasta],
        "with --graph": d + ["--graph", other, "--compare-to", other, "--pair-agreement", tmp_path / "agree.tsv"],
        "only with -T": d + ["--monomers-only", "-T", other, fasta],
        "only with --infer-tree": d + ["--monomers-only", "--infer-tree", fasta],
        "only with --pair-stats": d + ["--monomers-only", "--pair-stats", other, fasta],
        "only with -c": d + ["--monomers-only", "-c", fasta],
        "only with -t": d + ["--monomers-only", "-t", 2, fasta],
        "only with --force-gfa-output": d + ["--monomers-only", "--force-gfa-output", fasta],
        "only with -C": d + ["--monomers-only", "-C", other, fasta],
        "only with --dotplot": d + ["--monomers-only", "--dotplot", other, fasta],
        "only with --periods": d + ["--monomers-only", "--periods", other, fasta],
        "--dotplot-only with --monomers": ["--dotplot", other, "--dotplot-only"] + d + [fasta],
        "--periods-only with --monomers": ["--periods", other, "--periods-only"] + d + [fasta],
        "both -only options": ["--periods", other, "--periods-only"] + d + ["--monomers-only", fasta],
    }
    for opt, (least, most, fine) in NUMBERS.items():
        cases[opt + " not a number"] = d + [opt, "x", fasta]
        cases[opt + " a fraction"] = d + [opt, "2.5", fasta]
        cases[opt + " empty"] = d + [opt, "", fasta]
        cases[opt + " alone"] = [opt, fine, fasta]
        cases[opt + " above the limit"] = d + [opt, most + 1, fasta]
        cases[opt + " below the limit"] = d + [opt, least - 1, fasta]
    return cases


def test_cli_refusals(tmp_path, fasta, templates_fa):
    """each is one "error:" line and status 1 with nothing on standard output, before the FASTA is read or a device opened"""
    cases = refusals(tmp_path, fasta, templates_fa)
    assert len(cases) >= 70
    for name, args in cases.items():
        r = run_cli(args)
        err = r.stderr.decode().splitlines()
        assert r.returncode == 1 and r.stdout == b"", (name, r.returncode, r.stderr)
        assert len(err) == 1 and err[0].startswith("error: ") and "GPU" not in err[0], (name, err)
        for made in ("monomers.tsv", "summary.tsv", "other.tsv"):
            assert not (tmp_path / made).exists(), (name, made)
        assert (tmp_path / "old.tsv").read_text() == "keep me\n" and templates_fa.read_text().startswith(">m0\n"), name
    # the same refusals without a FASTA that could be read: they come first
    r = run_cli(["--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, "--monomers-chunk", 50, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"--monomers-chunk" in r.stderr and b"missing.fa" not in r.stderr
    r = run_cli(["--monomers", tmp_path / "monomers.tsv", "--monomers-templates", tmp_path / "missing_templates.fa", tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"missing_templates.fa" in r.stderr and b"missing.fa" not in r.stderr
    # the extreme values pass the option checks: the run then ends at the FASTA that is not there
    for pick in (0, 1):
        args = ["--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, "--monomers-summary", tmp_path / "summary.tsv", "--monomers-only",
                "--monomers-strands", ("forward", "both")[pick]]
        for opt, limits in NUMBERS.items():
            args += [opt, limits[pick]]
        r = run_cli(args + [tmp_path / "missing.fa"])
        assert r.returncode == 1 and b"missing.fa" in r.stderr and not (tmp_path / "monomers.tsv").exists(), r.stderr
    r = run_cli(["--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, "--monomers-chunk", 0, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"missing.fa" in r.stderr


def test_cli_generate_config_help_and_abbreviations(tmp_path, templates_fa):
    plain = run_cli(["-G"])
    with_options = run_cli(["-G", "--monomers", tmp_path / "monomers.tsv", "--monomers-templates", templates_fa, "--monomers-summary", tmp_path / "summary.tsv",
                            "--monomers-strands", "both", "--monomers-match", 2, "--monomers-mismatch", -3, "--monomers-insertion", -2, "--monomers-deletion", -2,
                            "--monomers-chunk", 128, "--monomers-overlap", 20])
    assert plain.returncode == 0 and with_options.returncode == 0 and plain.stdout == with_options.stdout and plain.stdout
    assert b"monomers" not in plain.stdout and not (tmp_path / "monomers.tsv").exists() and not (tmp_path / "summary.tsv").exists()
    text = run_cli(["-h"]).stderr.decode()
    for opt in ("--monomers FILE", "--monomers-templates FASTA", "--monomers-summary FILE", "--monomers-strands", "--monomers-match INT", "--monomers-mismatch INT",
                "--monomers-insertion INT", "--monomers-deletion INT", "--monomers-chunk INT", "--monomers-overlap INT", "--monomers-only"):
        assert opt in text, opt
    # the abbreviations of the options that begin with --m keep their meaning: --max-c is --max-count, --msa-o is --msa-out, --min-e is --min-event
    old = tmp_path / "old.tsv"
    old.write_text("keep me\n")
    r = run_cli(["--msa-o", old, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"MSA file already exists" in r.stderr
    r = run_cli(["--min-e", 5, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"--min-event needs --pair-events" in r.stderr
    r = run_cli(["--max-c", "x", tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"missing.fa" not in r.stderr
    r = run_cli(["--monomers", old, "--monomers-t", templates_fa, tmp_path / "missing.fa"])   # and the new ones have theirs
    assert r.returncode == 1 and b"Monomer decomposition file already exists" in r.stderr
