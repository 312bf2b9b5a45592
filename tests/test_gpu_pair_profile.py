"""Windowed pairwise profiles and gap events on the device: cl_induced_pairwise_profiles (induced_profile_kernel) and cl_induced_gap_events_batch
(induced_events_kernel) against the host functions pair by pair, against the Python walk of the device's own CIGAR text, and the command line's
--pair-profile / --pair-events against the -A files of the same run.  Every comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests import helpers as H
from tests import test_gpu_induced_pairs as tip
from tests import test_pair_profile as tpp
from tests import test_pair_stats as tps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
_faulted = []


def device_or_code(fn, *args):
    try:
        return fn(*args)
    except capi.ClError as e:
        return e.code


def check_all_pairs(ctx, g, windows, min_lens):
    """every ordered pair: the pairs the host function aligns in one batch per window / least length, each failing pair alone with the host's code"""
    n = len(g.path_off) - 1
    code = {p: tps.stat_or_code(g, *p) for p in tip.all_pairs(n)}
    pairs = [p for p in tip.all_pairs(n) if not isinstance(code[p], int)]
    for w in windows:
        got = capi.induced_pairwise_profiles(g, pairs, w, ctx)
        assert len(got) == len(pairs)
        for p, prof in zip(pairs, got):
            assert np.array_equal(prof, capi.induced_pairwise_profile(g, p[0], p[1], w)), (p, w)
    for m in min_lens:
        got = capi.induced_gap_events_batch(g, pairs, m, ctx)
        assert len(got) == len(pairs)
        for p, ev in zip(pairs, got):
            assert tpp.event_rows(ev) == tpp.event_rows(capi.induced_gap_events(g, p[0], p[1], m)), (p, m)
    for p in tip.all_pairs(n):
        if isinstance(code[p], int):
            assert device_or_code(capi.induced_pairwise_profiles, g, [p], windows[0], ctx) == code[p], p
            assert device_or_code(capi.induced_gap_events_batch, g, [p], min_lens[0], ctx) == code[p], p
    return n * n


@pytest.mark.gpu
def test_gpu_profiles_and_events_equal_host_on_msa_graphs(gpu_ctx):
    seen = 0
    for name, g in tip.golden_graphs():
        seen += check_all_pairs(gpu_ctx, g, (1, 64, 1000), (1, 10))
    rng = np.random.default_rng(5)
    for k in range(6):
        anc = "".join("ACGT"[b] for b in rng.integers(0, 4, int(rng.integers(50, 3000))))
        seen += check_all_pairs(gpu_ctx, synth.bubble_graph(anc, 4, seed=70 + k, alt_p=0.1, skip_p=0.05), (1, 3, 64, 1000), (1, 2, 5))
    assert seen > 2500


@pytest.mark.gpu
def test_gpu_profiles_and_events_equal_host_on_crafted_paths(gpu_ctx):
    """out-of-order and repeated meetings, 4 x 4 and 5 x 5 gap runs, empty and one-step paths; 30 000-step paths over many tiles of the kernel
    with runs crossing tile edges and window edges on and off the tile edges; the same pairs shuffled and repeated in one batch"""
    small, long = tps.crafted_graphs()
    n = len(small.path_off) - 1
    assert check_all_pairs(gpu_ctx, small, (1, 3, 7, 64, 1000), tpp.MIN_LENS) == n * n
    assert check_all_pairs(gpu_ctx, long, (1, 1000, 1024, 4096, 4097, 40000), tpp.MIN_LENS) == 16
    rng = np.random.default_rng(9)
    pairs = [tuple(int(x) for x in p) for p in rng.integers(0, n, (500, 2)) if int(p[0]) != 4]   # (path 4 repeats nodes: only a second path)
    got = capi.induced_pairwise_profiles(small, pairs, 7, gpu_ctx)
    assert all(np.array_equal(a, capi.induced_pairwise_profile(small, p, q, 7)) for a, (p, q) in zip(got, pairs))
    got = capi.induced_gap_events_batch(small, pairs, 1, gpu_ctx)
    assert [tpp.event_rows(e) for e in got] == [tpp.event_rows(capi.induced_gap_events(small, p, q, 1)) for p, q in pairs]
    assert capi.induced_pairwise_profiles(small, [], 7, gpu_ctx) == [] and capi.induced_gap_events_batch(small, [], 1, gpu_ctx) == []
    for fn in (capi.induced_pairwise_profiles, capi.induced_gap_events_batch):
        assert device_or_code(fn, small, [(0, 1)], 0, gpu_ctx) == -1


@pytest.mark.gpu
def test_gpu_long_deletion_and_trailing_runs(gpu_ctx):
    """path 2 skips 10 000 consecutive nodes of path 1 (one D run over more windows than a wave has lanes at 64 bases a window, and than the
    workgroup has threads at 1), ends in nodes of its own (a trailing insertion) and leaves the end of path 1 unmet (a trailing deletion, 3 000
    bases: more windows than the workgroup has threads at 1)"""
    rng = np.random.default_rng(21)
    n1 = 16000
    p1 = list(range(n1))
    p2 = p1[:700] + p1[10700:13000] + list(range(n1, n1 + 9))
    g = tip.path_graph(rng.integers(0, 4, n1 + 9), [p1, p2, p1[13000:]])
    assert capi.induced_pairwise_cigar(g, 0, 1) == b"700=10000D2300=3000D9I"
    for w in (64, 1, 63, 1000, 4096, 16000, 16001):
        for pair in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2)):
            got = capi.induced_pairwise_profiles(g, [pair], w, gpu_ctx)[0]
            assert np.array_equal(got, capi.induced_pairwise_profile(g, pair[0], pair[1], w)), (pair, w)
    assert tpp.event_rows(capi.induced_gap_events_batch(g, [(0, 1)], 9, gpu_ctx)[0]) == [(700, 700, 10000, 0), (13000, 3000, 3000, 0), (16000, 3000, 9, 1)]
    assert tpp.event_rows(capi.induced_gap_events_batch(g, [(0, 1)], 10, gpu_ctx)[0]) == [(700, 700, 10000, 0), (13000, 3000, 3000, 0)]


@pytest.mark.gpu
def test_gpu_batch_beyond_both_chunk_bounds(gpu_ctx):
    """2 600 pairs at one base a window: more pairs than a chunk holds (2 048) and about 520 MB of windows, twice what a chunk holds (256 MB)"""
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_24x7k.gfa.gz"), "rb").read()))[0]
    n = len(g.path_off) - 1
    rng = np.random.default_rng(3)
    pairs = [tuple(int(x) for x in p) for p in rng.integers(0, n, (2600, 2))]
    got = capi.induced_pairwise_profiles(g, pairs, 1, gpu_ctx)
    assert sum(len(a) for a in got) * 32 > (256 << 20)   # (about 520 MB)
    one = {p: capi.induced_pairwise_profile(g, p[0], p[1], 1) for p in set(pairs)}
    assert all(np.array_equal(a, one[p]) for a, p in zip(got, pairs))
    del got
    ev = capi.induced_gap_events_batch(g, pairs, 1, gpu_ctx)
    one = {p: tpp.event_rows(capi.induced_gap_events(g, p[0], p[1], 1)) for p in set(pairs)}
    assert [tpp.event_rows(e) for e in ev] == [one[p] for p in pairs]


@pytest.mark.gpu
def test_gpu_profiles_and_events_are_the_walk_of_the_devices_own_text(gpu_ctx):
    _, long = tps.crafted_graphs()
    pairs = [p for p in tip.all_pairs(4) if not isinstance(tps.stat_or_code(long, *p), int)]   # (path 1 may meet a drawn node twice)
    walks = [tpp.Walk(c) for c in capi.induced_pairwise_cigars(long, pairs, gpu_ctx)]
    assert len(pairs) >= 12
    for w in (1, 1000, 4097):
        got = capi.induced_pairwise_profiles(long, pairs, w, gpu_ctx)
        for (a, b), walk, prof in zip(pairs, walks, got):
            assert np.array_equal(prof, walk.profile(int(long.path_off[a + 1] - long.path_off[a]), w)), (a, b, w)
    for m in (1, 5):
        got = capi.induced_gap_events_batch(long, pairs, m, gpu_ctx)
        assert [tpp.event_rows(e) for e in got] == [walk.events(m) for walk in walks]


def run(args, cwd, timeout=900):
    if _faulted:
        pytest.fail("an earlier child of this module ended abnormally (%s): no further GPU process is started" % _faulted[0])
    try:
        r = subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired:
        _faulted.append("time limit of %d s" % timeout)
        raise
    if r.returncode < 0:
        _faulted.append("signal %d" % -r.returncode)
        pytest.fail("killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def read_tsv(path, header):
    text = open(path).read()
    lines = text.split("\n")
    assert text.endswith("\n") and lines[0].split("\t") == header.split()
    return [ln.split("\t") for ln in lines[1:-1]]


@pytest.mark.gpu
def test_gpu_cli_pair_profile_and_events(gpu_ctx, tmp_path):
    """--pair-profile, --pair-events and -A in one run: the rows are the Python walk of the .txt files of the same run, and standard output is
    what it is without the new options"""
    from tests.test_restart import case
    d = case()
    (tmp_path / "in.fa").write_bytes(bytes(d["fasta"]))
    (tmp_path / "t.nwk").write_text(str(d["newick"][0]))
    base = ["-v", 0, "-a", int(d["budget"][0]), "-T", "t.nwk"]
    plain = run(base + ["in.fa"], tmp_path)
    got = run(base + ["--pair-profile", "p.tsv", "--window", 300, "--pair-events", "e.tsv", "--min-event", 2, "-A", "pw", "in.fa"], tmp_path)
    assert got.stdout == plain.stdout and plain.stdout.startswith(b"H\t")
    _, names = capi.read_gfa(got.stdout, add_sentinels=True)
    walks = {}
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            walks[a, b] = tpp.Walk(open(os.path.join(tmp_path, "pw_%s_%s.txt" % (names[a], names[b])), "rb").read())
    want_p, want_e = [], []
    for (a, b), walk in walks.items():
        n1 = walk.end1   # path 2 meets path 1's nodes in order in an MSA graph: the walk ends at the end of path 1
        for w, row in enumerate(walk.profile(n1, 300).tolist()):
            want_p.append([names[a], names[b], str(w * 300), str(min((w + 1) * 300, n1))] + [str(v) for v in row])
        want_e += [[names[a], names[b], "DI"[op], str(i1), str(i2), str(n)] for i1, i2, n, op in walk.events(2)]
    assert read_tsv(tmp_path / "p.tsv", "sample1 sample2 window_start window_end matches mismatches insertions deletions") == want_p
    assert read_tsv(tmp_path / "e.tsv", "sample1 sample2 type pos1 pos2 length") == want_e
    assert len(want_p) > len(walks) and want_e
    # the defaults: 1 000 bases a window, events from 50 bases
    run(base + ["--pair-profile", "p2.tsv", "--pair-events", "e2.tsv", "in.fa"], tmp_path)
    rows = read_tsv(tmp_path / "p2.tsv", "sample1 sample2 window_start window_end matches mismatches insertions deletions")
    assert rows[0][2:4] == ["0", "1000"] or int(rows[0][3]) < 1000
    want = [[names[a], names[b], "DI"[op], str(i1), str(i2), str(n)] for (a, b), walk in walks.items() for i1, i2, n, op in walk.events(50)]
    assert read_tsv(tmp_path / "e2.tsv", "sample1 sample2 type pos1 pos2 length") == want
