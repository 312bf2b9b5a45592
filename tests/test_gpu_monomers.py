"""GPU suite: cl_monomer_decompose_compute (monomers_kernels.hip) == cl_monomer_decompose_host == the restatements of tests/test_monomers.py, every
field of every block.  Which case reaches which part of the device path:
  lane, wave and workgroup boundaries of the scan and of the diagonal exchange           test_template_lengths, test_mixed_template_lengths
  every cell count a lane can hold (CL_MONOMERS_CELLS forces one), up to 16 waves        the `cells` parameter of those and of the next two
  the largest template set, 8 192 bases                                                  test_largest_template_set
  the reduction across waves and its tie to the smallest m                               test_many_short_templates
  ties on the start at every cell                                                        test_ties_at_every_cell
  problems of 0, 1, C - 1, C, C + 1 and C + V + 1 rows, record batches of 64             test_sequence_lengths
  more problems than the persistent grid has workgroups (2 048)                          test_more_problems_than_workgroups
  one workgroup walking 20 000 rows, hundreds of record batches, the base prefetch       test_one_long_problem
Each case takes a second or two."""
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_gpu_device_memory import steady
from tests.test_monomers import BIN, HOR_CHUNKINGS, SCORE_SETS, params, problem_rows, problem_tuples, random_case, restated, revcomp, same_blocks, tsv_rows

pytestmark = pytest.mark.gpu


def check(ctx, seqs, templates, scores=(1, -1, -1, -1), chunk=0, overlap=0, strands=1, problem=problem_rows, want=None):
    """device == host == restatement; returns the restatement's blocks"""
    want, n_problems = want or restated(seqs, templates, scores, chunk, overlap, strands, problem)
    kw = params(scores, chunk=chunk, overlap=overlap, strands=strands)
    same_blocks(capi.monomer_decompose_host(seqs, templates, **kw), want, n_problems)
    got = capi.monomer_decompose(ctx, seqs, templates, **kw)
    same_blocks(got, want, n_problems)
    assert got["dp_ms"] >= 0 and got["trace_ms"] >= 0
    return want


def mutated(rng, text, rate=0.08):
    out = []
    for c in text:
        x = rng.random()
        if x < rate / 3:
            continue
        out.append("ACGT"[int(rng.integers(0, 4))] if x < rate else c)
        if x > 1 - rate / 3:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def random_template(rng, length):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, length))


@pytest.fixture(params=[None, 4, 8, 16, 24, 36], ids=lambda c: "cells=%s" % c)
def cells(request, monkeypatch):
    """the cells a lane holds: chosen by the library, or forced (a forced count that cannot hold the set leaves the choice to the library)"""
    if request.param is not None:
        monkeypatch.setenv("CL_MONOMERS_CELLS", str(request.param))
    return request.param


TEMPLATE_LENGTHS = [1, 63, 64, 65, 171, 255, 256, 257, 1024]
_single = {}


def single_case(length):
    """one template of `length` bases and two and a half mutated copies of it, the restatement computed once for every cell count"""
    if length not in _single:
        rng = np.random.default_rng(length)
        t = random_template(rng, length)
        seq = (mutated(rng, t[length // 2:]) + mutated(rng, t) + mutated(rng, t))[:max(40, min(2 * length + length // 2, 1400))]
        if length == 1:
            seq = (t * 7 + "N" + t * 3 + "acgt") * 3
        _single[length] = ([seq], [t], restated([seq], [t], problem=problem_rows))
    return _single[length]


@pytest.mark.parametrize("length", TEMPLATE_LENGTHS)
def test_template_lengths(gpu_ctx, cells, length):
    seqs, templates, want = single_case(length)
    check(gpu_ctx, seqs, templates, want=want)
    assert len(want[0]) >= 2


_mixed = []


def test_mixed_template_lengths(gpu_ctx, cells):
    if not _mixed:
        rng = np.random.default_rng(77)
        templates = [random_template(rng, n) for n in TEMPLATE_LENGTHS]
        seq = "".join(mutated(rng, templates[k]) for k in (4, 8, 2, 0, 7, 5, 1, 0, 3, 6, 4))
        _mixed.append(([seq], templates, restated([seq], templates, problem=problem_rows)))
    seqs, templates, want = _mixed[0]
    assert sum(len(t) for t in templates) == 2156
    check(gpu_ctx, seqs, templates, want=want)
    assert set(want[0]["monomer"].tolist()) >= {1, 2, 3, 4, 5, 6, 7, 8}


_largest = []


def test_largest_template_set(gpu_ctx, cells):
    if not _largest:
        rng = np.random.default_rng(8192)
        templates = [random_template(rng, 1024) for _ in range(8)]
        seq = mutated(rng, templates[7][700:]) + mutated(rng, templates[0][:300]) + mutated(rng, templates[3])[:500]
        _largest.append(([seq], templates, restated([seq], templates, problem=problem_rows)))
    seqs, templates, want = _largest[0]
    check(gpu_ctx, seqs, templates, want=want)
    with pytest.raises(capi.ClError) as e:
        capi.monomer_decompose(gpu_ctx, seqs, templates + ["A"])
    assert e.value.code == -1 and "templates" in str(e.value)


_short = []


def test_many_short_templates(gpu_ctx, cells):
    """400 templates of 5 bases, many of them equal: the best last cell is found in several waves at once and the smallest m must win"""
    if not _short:
        rng = np.random.default_rng(400)
        distinct = [random_template(rng, 5) for _ in range(40)]
        templates = [distinct[int(x)] for x in rng.integers(0, 40, 400)]
        seq = "".join(mutated(rng, templates[int(x)], 0.05) for x in rng.integers(0, 400, 100))
        _short.append(([seq, seq[:70]], templates, restated([seq, seq[:70]], templates, problem=problem_rows)))
    seqs, templates, want = _short[0]
    check(gpu_ctx, seqs, templates, want=want)
    first = {}
    for m, t in enumerate(templates):
        first.setdefault(t, m)
    assert all(first[templates[m]] == m for m in want[0]["monomer"].tolist()) and len(set(want[0]["monomer"].tolist())) > 20


def test_ties_at_every_cell(gpu_ctx, cells):
    want = check(gpu_ctx, ["A" * 3000], ["A", "AA", "AAA"], problem=problem_rows)
    assert len(want) == 3000 and not want["monomer"].any()
    for templates in (["AAA", "AA", "A"], ["AA", "AAA"]):
        check(gpu_ctx, ["A" * 500], templates, problem=problem_rows)


@pytest.mark.parametrize("V", [0, 1, 70])
def test_sequence_lengths(gpu_ctx, V):
    C = 64
    seq, templates = random_case(64 + V, length=C + V + 1)
    seqs = [seq[:n] for n in (0, 1, C - 1, C, C + 1, C + V + 1)]
    for chunk in (C, 0):
        want = check(gpu_ctx, seqs, templates, chunk=chunk, overlap=V, problem=problem_tuples)
        assert len(want) > 10
    check(gpu_ctx, [""], templates, chunk=0)
    check(gpu_ctx, ["", ""], templates, chunk=C)
    check(gpu_ctx, [], templates)


def test_more_problems_than_workgroups(gpu_ctx):
    rng = np.random.default_rng(5000)
    templates = ["ACG", "TTCA"]
    pool = templates + ["N", "GG"]
    seqs = ["".join(pool[int(x)] for x in rng.integers(0, 4, int(rng.integers(1, 4)))) for _ in range(5000)]
    want = check(gpu_ctx, seqs, templates, chunk=0, problem=problem_tuples)
    assert len(want) > 5000


def test_one_long_problem(gpu_ctx):
    seq = synth.hor_sequences(41, 25000, 1)[0][:20000]
    assert len(seq) == 20000
    want = check(gpu_ctx, [seq], synth.hor_monomers(41), chunk=0)
    assert 110 < len(want) < 125 and want["end"][-1] == 20000


@pytest.mark.parametrize("scores", SCORE_SETS)
def test_score_sets(gpu_ctx, scores):
    for seed in (1, 2):
        seq, templates = random_case(seed, n_templates=4, length=300)
        for strands in (1, 2):
            check(gpu_ctx, [seq, seq[50:120]], templates, scores, strands=strands, problem=problem_tuples)
        check(gpu_ctx, [seq], templates, scores, chunk=64, overlap=20, problem=problem_tuples)
    check(gpu_ctx, [synth.hor_sequences(5, 6000, 1)[0][300:1000]], synth.hor_monomers(5), scores)


def test_both_strands(gpu_ctx):
    seq, templates = synth.hor_sequences(5, 6000, 1)[0][:3000], synth.hor_monomers(5)
    flipped = seq[:1000] + revcomp(seq[1000:2000]) + seq[2000:]
    want = check(gpu_ctx, [flipped], templates, strands=2)
    inside = want[(want["start"] >= 1100) & (want["end"] <= 1900)]
    assert len(inside) >= 4 and (inside["monomer"] >= 12).all()
    check(gpu_ctx, [flipped], templates, strands=2, chunk=1024, overlap=400)


@pytest.fixture(scope="module")
def hor():
    seqs = synth.hor_sequences(5, 6000, 3)
    assert [len(s) for s in seqs] == [5998, 10128, 5996]
    return seqs, synth.hor_monomers(5)


@pytest.fixture(scope="module")
def hor_whole(hor):
    return restated(hor[0], hor[1], problem=problem_rows)


@pytest.mark.parametrize("chunk,overlap", [(0, 0)] + HOR_CHUNKINGS)
def test_hor_arrays(gpu_ctx, hor, hor_whole, chunk, overlap):
    """at these chunkings the chunked blocks equal the whole's (tests/test_monomers.py), so one restatement serves all four"""
    n_problems = sum((len(s) + chunk - 1) // chunk for s in hor[0]) if chunk else 3
    check(gpu_ctx, hor[0], hor[1], chunk=chunk, overlap=overlap, want=(hor_whole[0], n_problems))
    assert np.bincount(hor_whole[0]["sequence"]).tolist() == [35, 59, 35]


def test_monomers_return_their_device_memory(gpu_ctx, hor):
    seqs, templates = hor
    steady(gpu_ctx, "monomer_decompose, 3 arrays in 24 chunks", lambda: capi.monomer_decompose(gpu_ctx, seqs, templates, chunk=1024, overlap=256))
    steady(gpu_ctx, "monomer_decompose, both strands, unchunked", lambda: capi.monomer_decompose(gpu_ctx, seqs[:1], templates, chunk=0, strands=2))
    steady(gpu_ctx, "monomer_decompose, empty sequences", lambda: capi.monomer_decompose(gpu_ctx, ["", ""], templates, chunk=0))
    steady(gpu_ctx, "monomer_decompose, no sequence", lambda: capi.monomer_decompose(gpu_ctx, [], templates))
    steady(gpu_ctx, "monomer_decompose, chunk 63", lambda: capi.monomer_decompose(gpu_ctx, seqs, templates, chunk=63), -1)
    steady(gpu_ctx, "monomer_decompose, no template", lambda: capi.monomer_decompose(gpu_ctx, seqs, []), -1)


# ---------------------------------------------------------------- the command line, end to end ------------------------------------------------
_faulted = []


def run_cli(args, timeout=120):
    """a fresh child with its own time limit; after a child that ended by a signal or its time limit no further one is started"""
    if _faulted:
        pytest.fail("an earlier child of this module ended abnormally (%s): no further GPU process is started" % _faulted[0])
    try:
        r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired:
        _faulted.append("time limit of %d s" % timeout)
        raise
    if r.returncode < 0:
        _faulted.append("signal %d" % -r.returncode)
        pytest.fail("killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r


def test_cli_end_to_end(tmp_path):
    seqs = synth.hor_sequences(13, 5000, 3)
    assert [len(s) for s in seqs] == [908, 4997, 9089]
    templates = synth.hor_monomers(13)
    names = ["chr1/a", "b", "c"]   # named as --pair-stats names them: '/' becomes '_'
    shown = [nm.replace("/", "_") for nm in names]
    tnames = ["m%d" % k for k in range(12)]
    fa, tf = tmp_path / "in.fa", tmp_path / "monomers.fa"
    fa.write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs)))
    tf.write_text("".join(">%s some words\n%s\n%s\n" % (nm, t[:100], t[100:]) for nm, t in zip(tnames, templates)))
    kw = params((2, -3, -2, -2), chunk=1024, overlap=400, strands=2)
    opts = ["--monomers-templates", tf, "--monomers-strands", "both", "--monomers-match", 2, "--monomers-mismatch", -3, "--monomers-insertion", -2,
            "--monomers-deletion", -2, "--monomers-chunk", 1024, "--monomers-overlap", 400]
    want = capi.monomer_decompose_host(seqs, templates, **kw)
    tlens = [len(t) for t in templates]
    text = capi.monomers_tsv(want, shown, tnames, tlens, **kw)
    assert text == tsv_rows(want["blocks"], shown, tnames, tlens, 2) and want["n_blocks"] > 80
    only = run_cli(["--monomers", tmp_path / "only.tsv", "--monomers-summary", tmp_path / "only_summary.tsv", "--monomers-only"] + opts + [fa])
    assert only.returncode == 0 and only.stdout == b"", only.stderr
    assert (tmp_path / "only.tsv").read_bytes() == text
    assert (tmp_path / "only_summary.tsv").read_bytes() == capi.monomers_summary_tsv(want, shown, tnames, tlens, **kw)
    plain = run_cli([fa])
    assert plain.returncode == 0 and plain.stdout.startswith(b"H\t")
    beside = run_cli(["--monomers", tmp_path / "beside.tsv", "-v", 3] + opts + [fa])
    assert beside.returncode == 0 and beside.stdout == plain.stdout
    assert (tmp_path / "beside.tsv").read_bytes() == text
    assert b"problems" in beside.stderr and b"blocks" in beside.stderr and beside.stderr.count(b" ms") >= 2
    again = run_cli(["--monomers", tmp_path / "only.tsv", "--monomers-only"] + opts + [fa])
    assert again.returncode == 1 and again.stdout == b"" and again.stderr.startswith(b"error: ")
