"""GPU suite: cl_period_spectrum_compute (periods_kernels.hip) == cl_period_spectrum_host == the numpy restatement of tests/test_periods.py, every
array byte for byte.  Which case reaches which part of the device path:
  62-bit and 2-bit keys, empty windows and sequences, windows of one base               test_messy_sequences
  many windows, successors in a later window, segments longer than one pass (512)        test_hor_arrays
  every value of a wave in one bin                                                       test_worst_case_contention
  both sides of d = max_period, the smallest and the largest row (2 and 16 384 bins)     test_exact_tandem_array
  more windows than the persistent grid has workgroups (2 048), 9 000 total rows         test_more_windows_than_workgroups
  one workgroup looping hundreds of times over one segment                               test_one_long_window
  the rounds of the peak kernel's arg-max, its radius, both thresholds                   test_peak_parameters
Each case takes a second or two."""
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_gpu_device_memory import steady
from tests.test_periods import BIN, COUNTERS, cyclic_unit, hist_rows, identities, messy_case, restated, same_spectrum, tsv_rows

pytestmark = pytest.mark.gpu


def check(ctx, seqs, k, W, D, want=None, **kw):
    """device == host == restatement; returns the restatement"""
    want = want or restated(seqs, k, W, D, **kw)
    host = capi.period_spectrum_host(seqs, k=k, window=W, max_period=D, **kw)
    same_spectrum(host, want)
    got = capi.period_spectrum(ctx, seqs, k=k, window=W, max_period=D, **kw)
    same_spectrum(got, want)
    identities(got)
    assert got["links_ms"] >= 0 and got["hist_ms"] >= 0
    return want


@pytest.mark.parametrize("k", [1, 5, 11, 21, 31])
@pytest.mark.parametrize("W", [1, 64, 257, 2 ** 20])
def test_messy_sequences(gpu_ctx, k, W):
    seqs = messy_case(k, W)
    for D in (1, 50, 4096):
        want = check(gpu_ctx, seqs, k, W, D)
        assert (want["kmers"][:want["n_windows"]] == 0).any() and want["kmers"].sum() > 0


@pytest.fixture(scope="module")
def hor():
    seqs = synth.hor_sequences(5, 6000, 3)
    assert [len(s) for s in seqs] == [5998, 10128, 5996]
    return seqs


@pytest.mark.parametrize("W", [256, 2000, 2 ** 20])
@pytest.mark.parametrize("k", [4, 8])
def test_hor_arrays(gpu_ctx, hor, k, W):
    want = check(gpu_ctx, hor, k, W, 4096)
    assert want["kmers"][:want["n_windows"]].max() > 512 or W == 256   # a segment longer than one pass of the stride loop
    if W == 256:
        assert want["n_windows"] == 88 and want["links"][0] > 0   # the successors of the first window's k-mers lie in later windows
    top = want["peaks"][want["n_windows"] + 1][0]
    assert abs(int(top["period"]) - (2052 if k == 8 else 171)) <= (20 if k == 8 else 5)


@pytest.mark.parametrize("W", [2 ** 20, 100])
def test_worst_case_contention(gpu_ctx, W):
    one = check(gpu_ctx, ["A" * 5000], 3, W, 50)
    t = one["n_windows"]
    assert (one["kmers"][t], one["links"][t], one["last"][t]) == (4998, 4997, 1) and one["hist"][t, 1] == 4997   # every link in bin 1
    four = check(gpu_ctx, ["ACGT" * 2000], 3, W, 50)
    t = four["n_windows"]
    assert (four["kmers"][t], four["links"][t], four["last"][t]) == (7998, 7994, 4) and four["hist"][t, 4] == 7994
    check(gpu_ctx, ["A" * 5000, "ACGT" * 2000, "AC" * 700], 3, W, 3)   # "ACGT": every link is "far"


def test_exact_tandem_array(gpu_ctx):
    seq = cyclic_unit() * 100
    at = check(gpu_ctx, [seq], 8, 2 ** 20, 37)
    assert (at["links"][0], at["far"][0], at["last"][0]) == (3656, 0, 37) and at["peaks"][0].tolist() == [(37, 3656), (0, 0), (0, 0)]
    below = check(gpu_ctx, [seq], 8, 2 ** 20, 36)
    assert (below["links"][0], below["far"][0], below["last"][0]) == (0, 3656, 37) and below["peaks"][0].tolist() == [(0, 0)] * 3
    check(gpu_ctx, [seq, seq], 8, 1000, 37)
    check(gpu_ctx, [seq, "A" * 300], 8, 700, 1)   # the smallest row: two bins
    largest = check(gpu_ctx, [seq[:1500], "AC" * 400], 8, 2 ** 20, 16383, n_peaks=16, peak_radius=64)   # the largest row: 64 KiB
    assert largest["hist"].shape == (4, 16384) and largest["peaks"][0][0].tolist() == (37, 1456)


def test_more_windows_than_workgroups(gpu_ctx):
    """9 000 sequences of 5 .. 7 bases at k = 2, W = 4, D = 3: 18 000 windows, every second one nearly empty, 9 000 total rows"""
    rng = np.random.default_rng(9)
    seqs = ["".join("ACGT"[x] for x in rng.integers(0, 2, int(rng.integers(5, 8)))) for _ in range(9000)]
    want = check(gpu_ctx, seqs, 2, 4, 3)
    assert want["n_windows"] == 18000 and want["n_rows"] == 27000 and (want["kmers"][:18000] <= 4).all() and (want["kmers"][1:18000:2] <= 2).all()
    assert want["links"].sum() > 9000 and want["far"].sum() > 0 and (want["peaks"]["count"] > 0).sum() > 1000


def test_one_long_window(gpu_ctx):
    """one sequence of 200 000 bases in one window: the stride loop of one workgroup runs 391 times"""
    seq = max(synth.hor_sequences(41, 250000, 2), key=len)[:200000]
    assert len(seq) == 200000
    want = check(gpu_ctx, [seq], 8, 2 ** 20, 4096)
    assert want["n_windows"] == 1 and want["kmers"][0] > 199000 and want["links"][0] > 100000
    assert np.array_equal(want["hist"][0], want["hist"][1])


@pytest.mark.parametrize("kw", [dict(n_peaks=1), dict(n_peaks=16), dict(peak_radius=5), dict(peak_radius=64), dict(min_period=200), dict(min_count=1),
                                dict(min_count=1000)], ids=lambda kw: "%s=%d" % next(iter(kw.items())))
def test_peak_parameters(gpu_ctx, hor, kw):
    want = check(gpu_ctx, hor, 8, 2000, 4096, **kw)
    assert (want["peaks"]["count"] > 0).any()


def test_without_the_rows(gpu_ctx, hor):
    full = capi.period_spectrum(gpu_ctx, hor, k=8, window=256, max_period=4096)
    lean = capi.period_spectrum(gpu_ctx, hor, k=8, window=256, max_period=4096, want_hist=0)
    assert lean["hist"] is None and full["hist"] is not None
    same_spectrum(lean, full, hist=False)
    same_spectrum(lean, capi.period_spectrum_host(hor, k=8, window=256, max_period=4096, want_hist=0), hist=False)


def test_no_kmer_at_all(gpu_ctx):
    for seqs in (["NNNN", "", "AC"], ["", ""], ["N" * 300]):
        want = check(gpu_ctx, seqs, 3, 2, 5)
        assert want["kmers"].sum() == 0 and not want["hist"].any() and not want["peaks"]["count"].any()


def test_periods_return_their_device_memory(gpu_ctx, hor):
    steady(gpu_ctx, "period_spectrum, 88 windows", lambda: capi.period_spectrum(gpu_ctx, hor, k=8, window=256, max_period=4096))
    steady(gpu_ctx, "period_spectrum, the rows stay on the device", lambda: capi.period_spectrum(gpu_ctx, hor, k=8, window=256, max_period=4096, want_hist=0))
    steady(gpu_ctx, "period_spectrum, no k-mer at all", lambda: capi.period_spectrum(gpu_ctx, ["NNNN", "", "AC"], k=3, window=4))
    steady(gpu_ctx, "period_spectrum, k 32", lambda: capi.period_spectrum(gpu_ctx, hor, k=32), -1)
    steady(gpu_ctx, "period_spectrum, max_period 16384", lambda: capi.period_spectrum(gpu_ctx, hor, max_period=16384), -1)


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
    names = ["chr1/a", "b", "c"]   # named as --pair-stats names them: '/' becomes '_'
    lengths = [len(s) for s in seqs]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs)))
    shown = [nm.replace("/", "_") for nm in names]
    opts = ["--periods-k", 6, "--periods-window", 1500, "--periods-max", 3000, "--periods-peaks", 4, "--periods-radius", 2, "--periods-min-period", 3,
            "--periods-min-count", 3]
    want = capi.period_spectrum_host(seqs, k=6, window=1500, max_period=3000, n_peaks=4, peak_radius=2, min_period=3, min_count=3)
    assert capi.periods_tsv(want, shown, lengths) == tsv_rows(want, shown, lengths) and capi.periods_hist_tsv(want, shown, lengths) == hist_rows(want, shown, lengths)
    only = run_cli(["--periods", tmp_path / "only.tsv", "--periods-hist", tmp_path / "only_hist.tsv", "--periods-only"] + opts + [fa])
    assert only.returncode == 0 and only.stdout == b"", only.stderr
    assert (tmp_path / "only.tsv").read_bytes() == capi.periods_tsv(want, shown, lengths)
    assert (tmp_path / "only_hist.tsv").read_bytes() == capi.periods_hist_tsv(want, shown, lengths)
    for scope in ("sequences", "windows"):
        r = run_cli(["--periods", tmp_path / (scope + ".tsv"), "--periods-hist", tmp_path / (scope + "_hist.tsv"), "--periods-only", "--periods-scope", scope] + opts + [fa])
        assert r.returncode == 0 and r.stdout == b""
        assert (tmp_path / (scope + ".tsv")).read_bytes() == capi.periods_tsv(want, shown, lengths, scope)
        assert (tmp_path / (scope + "_hist.tsv")).read_bytes() == capi.periods_hist_tsv(want, shown, lengths, scope)
    plain = run_cli([fa])
    assert plain.returncode == 0 and plain.stdout.startswith(b"H\t")
    beside = run_cli(["--periods", tmp_path / "beside.tsv", "-v", 3] + opts + [fa])
    assert beside.returncode == 0 and beside.stdout == plain.stdout
    assert (tmp_path / "beside.tsv").read_bytes() == (tmp_path / "only.tsv").read_bytes()
    assert b"rows" in beside.stderr and b"links" in beside.stderr and beside.stderr.count(b" ms") >= 2
    again = run_cli(["--periods", tmp_path / "only.tsv", "--periods-only"] + opts + [fa])
    assert again.returncode == 1 and again.stdout == b"" and again.stderr.startswith(b"error: ")
