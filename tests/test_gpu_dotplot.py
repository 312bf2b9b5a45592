"""GPU suite: cl_kmer_dotplot_compute (dotplot_kernels.hip) == cl_kmer_dotplot_host == the numpy restatement of tests/test_dotplot.py, exactly:
win_off, distinct, the entries byte for byte, threshold_q and the identities to the bit.  Which case reaches which branch of the pair kernel:
  lists cut into LDS chunks (a list longer than the 8 192 entries a chunk holds)   test_lists_longer_than_a_chunk (k 12, lists of 131 061)
  a chunk edge between lists or inside one, several lists in one chunk             test_tile_edges at 64 (64 lists of ~250 entries: two chunks); the HOR cases (one chunk)
  partial tiles (fewer rows or columns than the tile holds)                        test_tile_edges (88 windows at 3, 7, 64), the messy cases
  diagonal tiles (b >= a inside the tile) and off-diagonal tiles                   every case with more than one tile: test_tile_edges at 1 .. 7
  empty windows inside a tile                                                      the messy cases (N runs, sequences shorter than k)
  more tiles than the persistent grid has workgroups, more than one batch          test_more_tiles_than_workgroups_and_batches
The restated cases stay near 400 windows; each case takes a second or two."""
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_dotplot import BIN, restated, same_plot, tsv_rows
from tests.test_gpu_device_memory import steady
from tests.test_gpu_tree_infer import messy_sequences

pytestmark = pytest.mark.gpu


def check(ctx, seqs, k, W, min_identity, pairs=0, want=None, **kw):
    """device == host == restatement; returns the restatement"""
    want = want or restated(seqs, k, W, min_identity, pairs)
    host = capi.kmer_dotplot_host(seqs, k=k, window=W, pairs=pairs, min_identity=min_identity)
    same_plot(host, want)
    got = capi.kmer_dotplot(ctx, seqs, k=k, window=W, pairs=pairs, min_identity=min_identity, **kw)
    same_plot(got, want)
    e = got["entries"]
    assert np.all(e["a"] <= e["b"])
    key = e["a"].astype(np.uint64) << np.uint64(32) | e["b"].astype(np.uint64)
    assert np.all(key[1:] > key[:-1])   # strictly ascending (a, b)
    return want


@pytest.mark.parametrize("k", [1, 5, 11, 21, 31])
@pytest.mark.parametrize("W", ["k", 64, 257])
def test_messy_sequences(gpu_ctx, k, W):
    """the inputs of tests/test_dotplot.py's host test (cut to their first bases for windows of k bases, as there), all pairs and pairs of one sequence"""
    seqs = messy_sequences(k)
    if W == "k":
        W = k
        seqs = [s[:max(40, 4 * k)] for s in seqs]
    for pairs in (0, 1):
        want = check(gpu_ctx, seqs, k, W, 86.0, pairs)
        assert len(want["entries"]) > 0 and (want["distinct"] == 0).any()


@pytest.fixture(scope="module")
def hor():
    seqs = synth.hor_sequences(5, 6000, 3)
    assert [len(s) for s in seqs] == [5998, 10128, 5996]
    return seqs


HOR_CASES = {(11, 256, 86.0): (548, 3916), (15, 500, 86.0): (383, 1035), (21, 1000, 86.0): (185, 276), (11, 256, 95.0): (466, 3916), (5, 64, 86.0): (2147, 60378)}
_hor_restated = {}


def hor_restated(hor, case):
    if case not in _hor_restated:
        _hor_restated[case] = restated(hor, *case)
    return _hor_restated[case]


@pytest.mark.parametrize("case", list(HOR_CASES))
def test_hor_arrays(gpu_ctx, hor, case):
    """both outcomes of the threshold occur in every case: a threshold that keeps everything or nothing cannot pass"""
    want = hor_restated(hor, case)
    kept, considered = len(want["entries"]), want["considered"]
    assert (kept, considered) == HOR_CASES[case] and 0 < kept < considered
    check(gpu_ctx, hor, *case, want=want)


def test_tile_edges(gpu_ctx, hor):
    case = (11, 256, 86.0)
    want = hor_restated(hor, case)
    assert want["n_windows"] == 88
    for tile in (1, 2, 3, 7, 64, 0):
        check(gpu_ctx, hor, *case, want=want, tile_windows=tile)
    with pytest.raises(capi.ClError) as e:
        capi.kmer_dotplot(gpu_ctx, hor, k=11, window=256, tile_windows=65)
    assert e.value.code == -1 and "tile_windows" in str(e.value)


def test_pairs_of_one_sequence(gpu_ctx, hor):
    case = (11, 256, 86.0)
    every = hor_restated(hor, case)
    off = every["win_off"]
    seq_of = lambda g: np.searchsorted(off, g, side="right") - 1
    e = every["entries"]
    same_seq = seq_of(e["a"]) == seq_of(e["b"])
    assert 0 < same_seq.sum() < len(e)
    for tile in (0, 5):
        got = capi.kmer_dotplot(gpu_ctx, hor, k=11, window=256, pairs="self", min_identity=86.0, tile_windows=tile)
        assert got["entries"].tobytes() == e[same_seq].tobytes()
    check(gpu_ctx, hor, *case, pairs=1)


@pytest.fixture(scope="module")
def long_pair():
    rng = np.random.default_rng(77)
    a = rng.integers(0, 4, 300000)
    b = a.copy()
    at = rng.choice(len(b), len(b) // 100, replace=False)
    b[at] = (b[at] + rng.integers(1, 4, len(at))) % 4
    return ["".join("ACGT"[x] for x in a), "".join("ACGT"[x] for x in b)]


def test_lists_longer_than_a_chunk(gpu_ctx, long_pair):
    """6 windows whose lists hold up to 131 061 entries: sixteen LDS chunks a list"""
    want = check(gpu_ctx, long_pair, 12, 131072, 0.0)
    assert want["n_windows"] == 6 and want["distinct"].max() > 100000 and len(want["entries"]) == 21
    check(gpu_ctx, long_pair, 12, 131072, 0.0, want=want, tile_windows=1)
    narrowed = check(gpu_ctx, long_pair, 12, 131072, 86.0)
    assert 6 < len(narrowed["entries"]) < 21


def test_the_largest_window_and_the_smallest_k(gpu_ctx, long_pair):
    want = check(gpu_ctx, long_pair, 1, 2 ** 20, 0.0)
    assert want["n_windows"] == 2 and want["distinct"].tolist() == [4, 4] and len(want["entries"]) == 3


def test_more_tiles_than_workgroups_and_batches(gpu_ctx):
    """what the pair phase derives from the tile count: the persistent grid (2 048 workgroups) and the batches of at most 2^24 window pairs (4 096
    tiles of 64 x 64).  9 000 sequences of 5 .. 7 bases at W = k = 4, pairs of one sequence: 9 000 tiles, 18 000 windows, every second one without
    a k-mer"""
    rng = np.random.default_rng(9)
    seqs = ["".join("ACGT"[x] for x in rng.integers(0, 2, int(rng.integers(5, 8)))) for _ in range(9000)]
    want = restated(seqs, 4, 4, 0.0, pairs=1)
    assert want["n_windows"] == 18000 and len(want["entries"]) > 9000 - 1
    for tile in (64, 0, 1):
        check(gpu_ctx, seqs, 4, 4, 0.0, pairs=1, want=want, tile_windows=tile)


def test_dotplot_returns_its_device_memory(gpu_ctx, hor):
    steady(gpu_ctx, "kmer_dotplot, 88 windows", lambda: capi.kmer_dotplot(gpu_ctx, hor, k=11, window=256))
    steady(gpu_ctx, "kmer_dotplot, pairs of one sequence in tiles of 3", lambda: capi.kmer_dotplot(gpu_ctx, hor, k=11, window=256, pairs=1, tile_windows=3))
    steady(gpu_ctx, "kmer_dotplot, no k-mer at all", lambda: capi.kmer_dotplot(gpu_ctx, ["NNNNNNNN", "", "AC"], k=3, window=4))
    steady(gpu_ctx, "kmer_dotplot, k 32", lambda: capi.kmer_dotplot(gpu_ctx, hor, k=32, window=256), -1)
    steady(gpu_ctx, "kmer_dotplot, window below k", lambda: capi.kmer_dotplot(gpu_ctx, hor, k=11, window=10), -1)


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
    fa = tmp_path / "in.fa"
    fa.write_text("".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs)))
    shown = [nm.replace("/", "_") for nm in names]
    opts = ["--dotplot-k", 11, "--dotplot-window", 256, "--dotplot-min-identity", 80]
    want = restated(seqs, 11, 256, 80.0)
    assert 0 < len(want["entries"]) < want["considered"]
    plain = run_cli([fa])
    assert plain.returncode == 0 and plain.stdout.startswith(b"H\t")
    beside = run_cli(["--dotplot", tmp_path / "beside.tsv", "-v", 3] + opts + [fa])
    assert beside.returncode == 0 and beside.stdout == plain.stdout
    assert (tmp_path / "beside.tsv").read_bytes() == tsv_rows(want, shown, seqs)
    assert b"windows" in beside.stderr and b"entries" in beside.stderr
    only = run_cli(["--dotplot", tmp_path / "only.tsv", "--dotplot-only"] + opts + [fa])
    assert only.returncode == 0 and only.stdout == b""
    assert (tmp_path / "only.tsv").read_bytes() == (tmp_path / "beside.tsv").read_bytes()
    own = run_cli(["--dotplot", tmp_path / "self.tsv", "--dotplot-only", "--dotplot-pairs", "self"] + opts + [fa])
    assert own.returncode == 0 and own.stdout == b""
    want_self = restated(seqs, 11, 256, 80.0, pairs=1)
    assert 0 < len(want_self["entries"]) < len(want["entries"])
    assert (tmp_path / "self.tsv").read_bytes() == tsv_rows(want_self, shown, seqs)
    again = run_cli(["--dotplot", tmp_path / "self.tsv", "--dotplot-only"] + opts + [fa])
    assert again.returncode == 1 and again.stdout == b"" and again.stderr.startswith(b"error: ")
