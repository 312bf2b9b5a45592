"""GPU suite: cl_strand_profile_compute (strands_kernels.hip) == cl_strand_profile_host, every array byte for byte, the votes included; the
intervals and the turned sequences of the device profile; centrolign-orient end to end.  Which case reaches which part of the device path:
  key widths 2 to 62 bits (one to eight passes of the sort), even k with palindromes                    test_messy_sequences
  windows of 1, 63, 64, 65, 1000 and 2^20 bases on lengths that are no multiple, a last window
  shorter than k, word-aligned and unaligned window starts                                              test_messy_sequences
  an empty sequence, one shorter than k, one of exactly k, runs of N, lower case                        test_messy_sequences
  runs of one key longer than a sort tile (2 048) that cross workgroups                                 test_long_runs
  300 sequences of 1 to 40 bases: the sequence search of positions and windows                          test_many_short_sequences
  no sequence, no base, no k-mer                                                                        test_nothing_to_do
Each case takes a second or two."""
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi
from tests.test_gpu_device_memory import steady
from tests.test_strands import BIN, check_recipe, recipe, revcomp, rows_of, same_profile

pytestmark = pytest.mark.gpu


def check(ctx, seqs, k, W):
    """device == host with and without the votes; returns the host profile"""
    want = capi.strand_profile_host(seqs, k=k, window=W)
    got = capi.strand_profile(ctx, seqs, k=k, window=W)
    same_profile(got, want)
    assert got["sort_ms"] >= 0 and got["vote_ms"] >= 0
    lean = capi.strand_profile(ctx, seqs, k=k, window=W, want_votes=0)
    same_profile(lean, dict(want, votes=None))
    return want


def messy_case(k, W):
    """texts over ACGTacgt with copies on both strands; an empty sequence, one shorter than k, one of exactly k, runs of N that break every k-mer
    of a stretch, lower case; lengths that are no multiple of the window, and (below 2^20) a last window shorter than k"""
    rng = np.random.default_rng(100 + k)
    def text(n):
        return "".join("ACGTacgt"[x] for x in rng.choice(8, n, p=[0.22] * 4 + [0.03] * 4))
    a, b = text(1201), text(777)
    seqs = [a, "", b[:k - 1], revcomp(a[100:900]).decode(), b[:k], a[50:950].lower(), b, "N" * 70 + b[100:400] + "NN" + revcomp(b[300:700]).decode() + "n" * 5,
            ("ACGTN" * 40)[:k * 6 + 3], revcomp(b).decode() + a[:131]]
    if W <= 1000:
        seqs.append(text(2 * W + max(k - 1, 1)))
    return seqs


@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 17, 21, 31])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 1000, 2 ** 20])
def test_messy_sequences(gpu_ctx, k, W):
    seqs = messy_case(k, W)
    want = check(gpu_ctx, seqs, k, W)
    assert want["forward"].sum() > 0 and want["reverse"].sum() > 0
    if k >= 4:
        assert (want["votes"] == 3).any()
    if k > 1:
        assert (want["kmers"] == 0).any()
        if 1 < W <= 1000:
            assert want["kmers"][-1] == 0 and want["kmers"][-2] == W   # the last window is shorter than k


@pytest.mark.parametrize("k", [1, 2, 12])
def test_long_runs(gpu_ctx, k):
    """A * 5000 + T * 3000 beside a second copy of A * 5000: the runs of one key are longer than a sort tile and cross workgroups.  The k - 1
    k-mers across the junction occur once each, as does the reverse complement of each: neutral"""
    seqs = ["A" * 5000 + "T" * 3000, "A" * 5000]
    for W in (1000, 4096):
        want = check(gpu_ctx, seqs, k, W)
        assert want["forward"].sum() == 2 * (5000 - k + 1) and want["reverse"].sum() == 3000 - k + 1 and want["distinct"] == {1: 1, 2: 2, 12: 7}[k]
    rows = rows_of(capi.strand_intervals(capi.strand_profile(gpu_ctx, seqs, k=k, window=1000)))
    assert len(rows) == 1 and rows[0][:4] == (0, 5000, 8000, 3)


def test_many_short_sequences(gpu_ctx):
    rng = np.random.default_rng(3)
    seqs = ["".join("ACGTN"[x] for x in rng.choice(5, int(rng.integers(1, 41)), p=[0.24] * 4 + [0.04])) for _ in range(300)]
    seqs[17] = seqs[250] = ""
    for k, W in ((2, 7), (3, 64), (5, 1)):
        want = check(gpu_ctx, seqs, k, W)
        assert want["n_seq"] == 300 and want["forward"].sum() > 0 and want["reverse"].sum() > 0


def test_nothing_to_do(gpu_ctx):
    for seqs in ([], [""], ["", ""], ["NNNN", "", "AC"], ["N" * 300]):
        want = check(gpu_ctx, seqs, 3, 2)
        assert want["kmers"].sum() == 0 and want["distinct"] == 0


@pytest.mark.parametrize("seed", range(3))
def test_recipe_on_the_device(gpu_ctx, seed):
    profile, iv = check_recipe(seed, lambda seqs: capi.strand_profile(gpu_ctx, seqs, k=21, window=1000))
    same_profile(profile, capi.strand_profile_host(recipe(seed)[1], k=21, window=1000))
    lean = capi.strand_profile(gpu_ctx, recipe(seed)[1], k=21, window=1000, want_votes=0)
    assert [row[0] for row in rows_of(capi.strand_intervals(lean))] == [row[0] for row in rows_of(iv)]


def test_strands_return_their_device_memory(gpu_ctx):
    seqs = recipe(0)[1]
    steady(gpu_ctx, "strand_profile, 4 x 20 kbp", lambda: capi.strand_profile(gpu_ctx, seqs, k=21, window=1000))
    steady(gpu_ctx, "strand_profile, the votes stay on the device", lambda: capi.strand_profile(gpu_ctx, seqs, k=21, window=1000, want_votes=0))
    steady(gpu_ctx, "strand_profile, no k-mer at all", lambda: capi.strand_profile(gpu_ctx, ["NNNN", "", "AC"], k=3, window=4))
    steady(gpu_ctx, "strand_profile, k 32", lambda: capi.strand_profile(gpu_ctx, seqs, k=32), -1)


# ---------------------------------------------------------------- the command line, end to end ------------------------------------------------
def test_cli_end_to_end(tmp_path):
    orig, mod, i, truth, j = recipe(0)
    names = ["chr1/a", "b", "c", "d"]   # shown as --pair-stats of centrolign names them: '/' becomes '_'
    fa = tmp_path / "in.fa"
    fa.write_bytes(b"".join(b">%s\n%s\n" % (nm.encode(), s) for nm, s in zip(names, mod)))
    host = capi.strand_profile_host(mod, k=21, window=1000)
    shown = [nm.replace("/", "_") for nm in names]
    r = subprocess.run([BIN, "--profile", str(tmp_path / "profile.tsv"), "--fasta-out", str(tmp_path / "fixed.fa"), "-v", "3", str(fa)], capture_output=True, timeout=120,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    assert r.stdout == capi.strand_intervals_tsv(capi.strand_intervals(host), shown)
    assert (tmp_path / "fixed.fa").read_bytes() == b"".join(b">%s\n%s\n" % (nm.encode(), s) for nm, s in zip(names, orig))   # seed 0 comes back to the base
    assert (tmp_path / "profile.tsv").read_bytes() == capi.strand_profile_tsv(host, shown)
    assert b"windows" in r.stderr and b"distinct" in r.stderr and b"intervals" in r.stderr and r.stderr.count(b" ms") == 2
