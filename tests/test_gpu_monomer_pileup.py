"""GPU suite: cl_monomer_pileup_compute (monomer_pileup_kernels.hip) == cl_monomer_pileup_host, every byte of every array, and
cl_monomer_templates_refine_compute == _host.  (tests/test_monomer_pileup.py holds the host against a restatement in Python.)  Which case reaches
which part of the device path:
  the lane that holds a template's last column, its cell in the lane, rows that start and end inside the wavefront   test_template_lengths
  every count of cells a lane can hold (CL_MONOMER_PILEUP_CELLS forces one that covers the template)                 the `cells` of its cases
  blocks of 1, L, 2 L and 2 L + 1 bases, of N alone, both strands, the three classes at three least_share            the same cases
  the direction bits in LDS and in the global slab (CL_MONOMER_PILEUP_BITS=global; 1 024 columns need the slab)      test_direction_bits_in_global_memory
  more blocks than resident waves, runs of one template that end inside a wave's range                               test_many_tiny_blocks
  no used block at all                                                                                               test_every_block_partial
Each case takes a second or less."""
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_gpu_device_memory import steady
from tests.test_gpu_monomers import mutated, random_template
from tests.test_monomer_pileup import PILEUP_HEADER, dec_of
from tests.test_monomers import BIN, SCORE_SETS, params, revcomp

pytestmark = pytest.mark.gpu
ARRAYS = ("col_off", "columns", "slots", "used", "partial", "long_", "weak", "score_sum")


def check(ctx, seqs, templates, dec, least_share=0, scores=(1, -1, -1, -1), **kw):
    """device == host in every array; returns the host's pileup"""
    kw = params(scores, **kw)
    want = capi.monomer_pileup_host(seqs, templates, dec, least_share, **kw)
    got = capi.monomer_pileup(ctx, seqs, templates, dec, least_share, **kw)
    for name in ARRAYS:
        if not np.array_equal(got[name], want[name]):
            at = np.argwhere(got[name] != want[name])[0]
            raise AssertionError("%s differs at %s: got %s, want %s" % (name, at.tolist(), got[name][tuple(at)], want[name][tuple(at)]))
    assert got["align_ms"] >= 0 and got["count_ms"] >= 0
    return want


TEMPLATE_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 171, 1023, 1024]
CELLS = [1, 2, 3, 4, 8, 16]
LENGTH_CASES = [(L, None) for L in TEMPLATE_LENGTHS] + [(L, R) for L in TEMPLATE_LENGTHS for R in CELLS if R * 64 >= L]
_length_input = {}


def length_input(L):
    """one template of L bases; blocks of 1, L, 2 L (used) and 2 L + 1 (long) bases on both strands, one of N alone, written by hand"""
    if L not in _length_input:
        rng = np.random.default_rng(1000 + L)
        t = random_template(rng, L)

        def copy_of(length, minus=False):
            text = mutated(rng, t)
            while len(text) < length:
                text += mutated(rng, t)
            return revcomp(text[:length]) if minus else text[:length]
        pieces = [(copy_of(1), 0, 0), (copy_of(L), 0, L), (copy_of(2 * L), 0, L), (copy_of(2 * L + 1), 0, L), ("N" * L, 0, 0), (copy_of(L, True), 1, L // 2),
                  (copy_of(2 * L, True), 1, 0), (copy_of(1, True), 1, L), (copy_of(L), 0, L // 3), ("n" * (2 * L), 1, L), (copy_of(L), 0, L)]
        seq, blocks = "", []
        for k, (text, monomer, score) in enumerate(pieces):
            blocks.append((0, len(seq), len(seq) + len(text), monomer, score, 1 if k == len(pieces) - 1 else 0))
            seq += text
        _length_input[L] = ([seq], [t], dec_of(blocks, 1))
    return _length_input[L]


@pytest.mark.parametrize("L,cells", LENGTH_CASES)
def test_template_lengths(gpu_ctx, monkeypatch, L, cells):
    if cells is not None:
        monkeypatch.setenv("CL_MONOMER_PILEUP_CELLS", str(cells))
    seqs, templates, dec = length_input(L)
    want = check(gpu_ctx, seqs, templates, dec, 0, strands=2)
    assert (want["used"][0], want["long_"][0], want["partial"][0], want["weak"][0]) == (9, 1, 1, 0)
    want = check(gpu_ctx, seqs, templates, dec, 400, strands=2)
    assert want["weak"][0] >= 3 and want["used"][0] >= 3
    want = check(gpu_ctx, seqs, templates, dec, 1000, strands=2)
    assert want["used"][0] == 4 and (want["columns"].sum(axis=1) == 4).all()


@pytest.mark.parametrize("L", [2, 171, 1024])
def test_direction_bits_in_global_memory(gpu_ctx, monkeypatch, L):
    """1 024 columns and a block of 2 048 bases need the slab anyway; the shorter ones are sent there"""
    monkeypatch.setenv("CL_MONOMER_PILEUP_BITS", "global")
    seqs, templates, dec = length_input(L)
    check(gpu_ctx, seqs, templates, dec, 0, strands=2)


def test_one_base_against_1024_columns_and_two_against_one(gpu_ctx):
    t = random_template(np.random.default_rng(3), 1024)
    want = check(gpu_ctx, [t[500]], [t], dec_of([(0, 0, 1, 0, 0, 0)], 1))
    assert want["columns"][:, 5].sum() == 1023 and want["score_sum"][0] == 1 - 1023
    want = check(gpu_ctx, ["AC", "CA", "NN"], ["A"], dec_of([(0, 0, 2, 0, 0, 0), (1, 0, 2, 0, 0, 0), (2, 0, 2, 0, 0, 0), (2, 1, 1, 0, 0, 0)], 3))
    assert want["columns"].tolist() == [[2, 0, 0, 0, 1, 1]] and want["slots"].tolist() == [[0, 1, 0, 0, 1], [0, 1, 0, 0, 0]] and want["score_sum"][0] == 0 + 0 - 2 - 1


def test_mixed_template_lengths(gpu_ctx):
    rng = np.random.default_rng(77)
    templates = [random_template(rng, n) for n in (1, 63, 65, 171, 5, 300)]
    order = [3, 5, 2, 0, 1, 4, 3, 3, 5, 1, 2, 4, 0, 5]
    seq, blocks = "", []
    for k, m in enumerate(order):
        text = mutated(rng, templates[m]) or "A"
        minus = k % 3 == 1
        blocks.append((0, len(seq), len(seq) + len(text), m + 6 if minus else m, len(templates[m]) // 2, 0))
        seq += revcomp(text) if minus else text
    want = check(gpu_ctx, [seq], templates, dec_of(blocks, 1), strands=2)
    assert want["used"].tolist() == [order.count(m) for m in range(6)]


def test_many_tiny_blocks(gpu_ctx):
    """5 000 blocks of 1 to 6 bases over three templates: more than the waves that are resident, and every wave's range crosses a template"""
    rng = np.random.default_rng(5000)
    templates = ["ACG", "TTCA", "G"]
    seq = "".join("ACGTN"[int(x)] for x in rng.choice(5, 20000, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    blocks, at = [], 0
    for k in range(5000):
        n = int(rng.integers(1, 7))
        if at + n > len(seq):
            at = 0
        blocks.append((0, at, at + n, int(rng.integers(0, 6)), int(rng.integers(0, 4)), 0))
        at += int(rng.integers(0, n + 1))
    want = check(gpu_ctx, [seq], templates, dec_of(blocks, 1), strands=2)
    assert want["used"].sum() > 3000 and want["long_"].sum() > 200
    check(gpu_ctx, [seq], templates, dec_of(blocks, 1), 700, strands=2)


def test_every_block_partial(gpu_ctx):
    seqs, templates, dec = length_input(171)
    dec = dict(dec, blocks=dec["blocks"].copy())
    dec["blocks"]["flags"] = [1, 2, 3] * 3 + [1, 2]
    want = check(gpu_ctx, seqs, templates, dec, strands=2)
    assert want["partial"][0] == 11 and not want["columns"].any() and not want["slots"].any() and want["score_sum"][0] == 0
    check(gpu_ctx, [], templates, dec_of([], 0))
    check(gpu_ctx, ["", ""], templates, dec_of([], 2))


@pytest.fixture(scope="module")
def hor():
    return synth.hor_sequences(5, 6000, 3), synth.hor_monomers(5)


@pytest.mark.parametrize("bits", ["lds", "global"])
def test_hor_arrays(gpu_ctx, monkeypatch, hor, bits):
    monkeypatch.setenv("CL_MONOMER_PILEUP_BITS", bits)
    seqs, templates = hor
    for kw in (dict(chunk=0), dict(chunk=4096, overlap=512)):
        dec = capi.monomer_decompose_host(seqs, templates, **kw)
        want = check(gpu_ctx, seqs, templates, dec, **kw)
        assert want["used"].sum() + want["partial"].sum() + want["long_"].sum() == 129 and want["used"].sum() > 100
    flipped = [seqs[0], revcomp(seqs[1]), seqs[2]]
    dec = capi.monomer_decompose_host(flipped, templates, chunk=0, strands=2)
    want = check(gpu_ctx, flipped, templates, dec, 500, chunk=0, strands=2)
    assert want["used"].sum() > 100 and want["slots"].sum() > 0


@pytest.mark.parametrize("scores", SCORE_SETS)
def test_score_sets(gpu_ctx, hor, scores):
    seqs, templates = [hor[0][0][300:2000], revcomp(hor[0][2][:900])], hor[1]
    dec = capi.monomer_decompose_host(seqs, templates, **params(scores, chunk=0, strands=2))
    want = check(gpu_ctx, seqs, templates, dec, 0, scores, chunk=0, strands=2)
    assert want["used"].sum() >= 10
    check(gpu_ctx, seqs, templates, dec, 600, scores, chunk=0, strands=2)


def test_refinement_equals_the_host_on_the_recovery_input(gpu_ctx):
    import random
    seqs, truth = synth.hor_sequences(5, 40000, 2), synth.hor_monomers(5)
    rng = random.Random(99)
    start = ["".join(synth._mut_track(rng, list(t), 0.05)[0]) for t in truth]
    want = capi.monomer_templates_refine_host(seqs, start, max_rounds=4)
    got = capi.monomer_templates_refine(gpu_ctx, seqs, start, max_rounds=4)
    assert got["templates"] == want["templates"] == truth and got["changed"] == want["changed"] and (got["rounds"], got["converged"]) == (want["rounds"], want["converged"]) == (2, True)
    counts = lambda r: [(q["blocks"], q["used"], q["changed"]) for q in r["round"]]
    assert counts(got) == counts(want) and all(q["dp_ms"] > 0 and q["align_ms"] > 0 for q in got["round"]) and not any(q["dp_ms"] or q["align_ms"] for q in want["round"])


def test_refinement_of_seeds_equals_the_host(gpu_ctx, hor):
    seqs = hor[0]
    seeds = capi.monomer_seed_templates(seqs, 171, 3, 5)["templates"]
    for kw in (dict(strands=1), dict(strands=2, least_share=300)):
        want = capi.monomer_templates_refine_host(seqs, seeds, max_rounds=3, **kw)
        got = capi.monomer_templates_refine(gpu_ctx, seqs, seeds, max_rounds=3, **kw)
        for key in ("templates", "changed", "rounds", "converged"):
            assert got[key] == want[key], key
        assert [(q["blocks"], q["used"], q["changed"]) for q in got["round"]] == [(q["blocks"], q["used"], q["changed"]) for q in want["round"]]


def test_pileup_and_refinement_return_their_device_memory(gpu_ctx, monkeypatch, hor):
    seqs, templates = hor
    dec = capi.monomer_decompose_host(seqs, templates)
    bad = dec_of([(0, 0, 7000, 0, 4, 0)], 3)
    steady(gpu_ctx, "monomer_pileup, 3 arrays", lambda: capi.monomer_pileup(gpu_ctx, seqs, templates, dec))
    steady(gpu_ctx, "monomer_pileup, no used block", lambda: capi.monomer_pileup(gpu_ctx, seqs, templates, dec, 1000))
    steady(gpu_ctx, "monomer_pileup, a block beyond its sequence", lambda: capi.monomer_pileup(gpu_ctx, seqs, templates, bad), -1)
    steady(gpu_ctx, "monomer_pileup, least_share 1001", lambda: capi.monomer_pileup(gpu_ctx, seqs, templates, dec, 1001), -1)
    steady(gpu_ctx, "monomer_templates_refine, 2 rounds", lambda: capi.monomer_templates_refine(gpu_ctx, seqs, templates, max_rounds=2))
    steady(gpu_ctx, "monomer_templates_refine, max_rounds 65", lambda: capi.monomer_templates_refine(gpu_ctx, seqs, templates, max_rounds=65), -1)
    steady(gpu_ctx, "monomer_templates_refine, chunk 63", lambda: capi.monomer_templates_refine(gpu_ctx, seqs, templates, chunk=63), -1)
    monkeypatch.setenv("CL_MONOMER_PILEUP_BITS", "global")
    steady(gpu_ctx, "monomer_pileup, the slab", lambda: capi.monomer_pileup(gpu_ctx, seqs, templates, dec))


# ---------------------------------------------------------------- the command line, end to end ------------------------------------------------
def test_cli_end_to_end(tmp_path, hor):
    """one child with its own time limit"""
    seqs, templates = hor
    names, tnames = ["chr1/a", "b", "c"], ["m%d" % k for k in range(12)]
    shown = [nm.replace("/", "_") for nm in names]
    fa, tf = tmp_path / "in.fa", tmp_path / "monomers.fa"
    fa.write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs)))
    tf.write_text("".join(">%s\n%s\n" % (nm, t) for nm, t in zip(tnames, templates)))
    refined = capi.monomer_templates_refine_host(seqs, templates, max_rounds=3, least_share=200)
    final = refined["templates"]
    assert refined["rounds"] == 2 and refined["converged"] and final != templates
    dec = capi.monomer_decompose_host(seqs, final)
    pile = capi.monomer_pileup_host(seqs, final, dec, 200)
    r = subprocess.run([BIN, "--monomers", str(tmp_path / "out.tsv"), "--monomers-templates", str(tf), "--monomers-rounds", "3", "--monomers-least-share", "200",
                        "--monomers-write-templates", str(tmp_path / "new.fa"), "--monomers-pileup", str(tmp_path / "pileup.tsv"), "--monomers-only", "-v", "3", str(fa)],
                       capture_output=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    assert (tmp_path / "new.fa").read_bytes() == capi.monomer_templates_fasta(tnames, final)
    assert (tmp_path / "out.tsv").read_bytes() == capi.monomers_tsv(dec, shown, tnames, [len(t) for t in final])
    text = (tmp_path / "pileup.tsv").read_bytes()
    assert text == capi.monomer_pileup_tsv(pile, tnames, final) and text.startswith(PILEUP_HEADER.encode())
    assert r.stderr.count(b"Template round") == 2 and b"129 blocks" in r.stderr and b"2 templates changed" in r.stderr and b"converged after 2 round(s)" in r.stderr
