"""Windowed pairwise profiles and gap events without a device: cl_induced_pairwise_profile and cl_induced_gap_events against a Python walk of
cl_induced_pairwise_cigar's text (the definitions of include/centrolign_amd.h restated here), their invariants against cl_induced_pairwise_stat,
and the command-line options that are refused before anything is read or opened."""
import gzip
import os
import re

import numpy as np
import pytest

from centrolign_amd import capi
from tests import helpers as H
from tests import test_gpu_induced_pairs as tip
from tests import test_pair_stats as tps

WINDOWS = (1, 3, 64, 1000)      # and n1, n1 + 1 of each pair
MIN_LENS = (1, 2, 5, 10 ** 9)


class Walk:
    """the CIGAR read left to right with i1 = i2 = 0: '=' and 'X' advance both, 'D' i1, 'I' i2"""

    def __init__(self, text):
        text = text.decode() if isinstance(text, bytes) else str(text)
        runs = re.findall(r"(\d+)([=XID])", text.strip())
        assert "".join(n + c for n, c in runs) == text.strip()
        self.runs = []              # (op, len, i1, i2 at the run's first column)
        i1 = i2 = 0
        for n, c in runs:
            n = int(n)
            self.runs.append((c, n, i1, i2))
            i1 += n if c != "I" else 0
            i2 += n if c != "D" else 0
        self.end1, self.end2 = i1, i2
        # per letter the value of i1 in front of every column
        self.col_i1 = {}
        for c in "=XID":
            start = np.array([r[2] for r in self.runs if r[0] == c], np.int64)
            length = np.array([r[1] for r in self.runs if r[0] == c], np.int64)
            at = np.repeat(start, length)
            if c != "I" and len(at):
                at = at + np.arange(len(at)) - np.repeat(np.cumsum(length) - length, length)
            self.col_i1[c] = at

    def profile(self, n1, window):
        """[n_win, 4]: the columns of '=', 'X', 'I', 'D' per window; a column belongs to window min(i1 // window, n_win - 1)"""
        n_win = max(1, -(-n1 // window))
        return np.stack([np.bincount(np.minimum(self.col_i1[c] // window, n_win - 1), minlength=n_win) for c in "=XID"], axis=1).astype(np.uint64)

    def events(self, min_len):
        """(pos1, pos2, len, op) of every I or D run of at least min_len columns, in order; op 0: D, 1: I"""
        return [(i1, i2, n, 1 if c == "I" else 0) for c, n, i1, i2 in self.runs if c in "ID" and n >= min_len]


def event_rows(ev):
    assert not ev["reserved"].any()
    return [(int(e["pos1"]), int(e["pos2"]), int(e["len"]), int(e["op"])) for e in ev]


def host_or_code(fn, *args):
    try:
        return fn(*args)
    except capi.ClError as e:
        return e.code


def windows_of(n1):
    return sorted(set(WINDOWS) | {max(n1, 1), n1 + 1})


def check_every_ordered_pair(g):
    n = len(g.path_off) - 1
    failing = 0
    for a, b in tip.all_pairs(n):
        n1 = int(g.path_off[a + 1] - g.path_off[a])
        cigar = tip.host_or_code(g, a, b)
        if isinstance(cigar, int):
            assert host_or_code(capi.induced_pairwise_profile, g, a, b, 7) == cigar, (a, b)
            assert host_or_code(capi.induced_gap_events, g, a, b, 1) == cigar, (a, b)
            failing += 1
            continue
        walk = Walk(cigar)
        stat = capi.induced_pairwise_stat(g, a, b)
        for w in windows_of(n1):
            got = capi.induced_pairwise_profile(g, a, b, w)
            assert got.shape == (max(1, -(-n1 // w)), 4) and got.dtype == np.uint64, (a, b, w)
            assert np.array_equal(got, walk.profile(n1, w)), (a, b, w)
            assert [int(v) for v in got.sum(axis=0)] == [stat[k] for k in capi.PAIR_WINDOW_FIELDS], (a, b, w)
        for m in MIN_LENS:
            assert event_rows(capi.induced_gap_events(g, a, b, m)) == walk.events(m), (a, b, m)
        ops = [e[3] for e in walk.events(1)]
        assert (ops.count(1), ops.count(0)) == (stat["ins_runs"], stat["del_runs"]), (a, b)
        assert walk.events(10 ** 9) == []
    return n * n, failing


def test_profile_and_events_equal_the_walk_on_the_golden_msa_graphs():
    seen = 0
    for name, g in tip.golden_graphs():
        if name == "wide_merge_50x5k":
            continue   # the test below
        seen += check_every_ordered_pair(g)[0]
    assert seen >= 10


def test_profile_and_events_equal_the_walk_on_the_50_path_root():
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_50x5k.gfa.gz"), "rb").read()))[0]
    assert check_every_ordered_pair(g) == (2500, 0)


def test_profile_and_events_on_the_crafted_paths():
    """out-of-order and repeated meetings (path-1 indices past path 1's end go to the last window), 4 x 4 and 5 x 5 gap runs, empty and one-step
    paths; 30 000-step paths"""
    small, long = tps.crafted_graphs()
    seen, failing = check_every_ordered_pair(small)
    assert seen == 144 and failing == 12   # path 4 repeats nodes: it cannot be a first path
    assert check_every_ordered_pair(long)[0] == 16
    # the cases by hand: 5 deletions against 5 insertions are two events, the D first, at the same pos2; 4 against 4 are mismatches
    assert capi.induced_pairwise_cigar(small, 0, 1).endswith(b"5D5I5=")
    assert event_rows(capi.induced_gap_events(small, 0, 1, 1)) == [(30, 30, 5, 0), (35, 30, 5, 1)]
    assert event_rows(capi.induced_gap_events(small, 0, 1, 6)) == []
    # an empty first path: one window that holds the insertions; an empty second path: the deletions window by window
    assert capi.induced_pairwise_profile(small, 5, 0, 10).tolist() == [[0, 0, 40, 0]]
    assert capi.induced_pairwise_profile(small, 0, 5, 16).tolist() == [[0, 0, 0, 16], [0, 0, 0, 16], [0, 0, 0, 8]]
    assert event_rows(capi.induced_gap_events(small, 0, 5, 40)) == [(0, 0, 40, 0)]
    assert capi.induced_pairwise_profile(small, 5, 5, 1).tolist() == [[0, 0, 0, 0]] and len(capi.induced_gap_events(small, 5, 5, 1)) == 0


def test_a_trailing_insertion_lies_in_the_last_window():
    g = tip.path_graph([0, 1, 2, 3] * 5, [[0, 1, 2, 3, 4, 5], [10, 11, 0, 1, 12, 13, 14, 2, 3, 4, 5, 15, 16, 17]])
    assert capi.induced_pairwise_cigar(g, 0, 1) == b"2I2=3I4=3I"
    # an I column lies in the window of the path-1 base it stands in front of
    assert capi.induced_pairwise_profile(g, 0, 1, 2).tolist() == [[2, 0, 2, 0], [2, 0, 3, 0], [2, 0, 3, 0]]
    assert capi.induced_pairwise_profile(g, 0, 1, 4).tolist() == [[4, 0, 5, 0], [2, 0, 3, 0]]
    assert event_rows(capi.induced_gap_events(g, 0, 1, 3)) == [(2, 4, 3, 1), (6, 11, 3, 1)]


def test_error_codes_follow_the_cigar_function():
    labels = [0, 1, 2, 3] * 5
    g = tip.path_graph(labels, [[0, 1, 2, 1, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])   # path 0 visits node 1 twice
    bad = tip.path_graph(labels, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    bad.path_nodes[4] = 1000
    codes = set()
    for graph, pairs in ((g, [(0, 1), (1, 0), (1, 9), (9, 1), (0, 0)]), (bad, [(1, 0), (0, 1), (0, 2), (1, 1)])):
        for a, b in pairs:
            want = tip.host_or_code(graph, a, b)
            for got in (host_or_code(capi.induced_pairwise_profile, graph, a, b, 2), host_or_code(capi.induced_gap_events, graph, a, b, 1)):
                assert isinstance(got, int) == isinstance(want, int) and (not isinstance(want, int) or got == want), (a, b)
            if isinstance(want, int):
                codes.add(want)
    assert codes == {-1, -7}   # CL_ERR_INVALID_ARGUMENT, CL_ERR_CYCLIC_GRAPH
    assert host_or_code(capi.induced_pairwise_profile, g, 1, 2, 0) == -1
    assert host_or_code(capi.induced_gap_events, g, 1, 2, 0) == -1
    assert len(capi.induced_pairwise_profile(g, 1, 2, 2 ** 64 - 1)) == 1


def test_the_new_symbols_are_exported():
    lib = capi.load_library()
    for sym in ("cl_induced_pairwise_profile", "cl_induced_pairwise_profiles", "cl_induced_gap_events", "cl_induced_gap_events_batch"):
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert capi.GAP_EVENT_DTYPE.itemsize == 32


# ---------------------------------------------------------------- the command line ----------------------------------------------------------
def test_cli_refuses_before_reading_anything(tmp_path):
    """none of these names an input that exists: a refusal that came after reading the FASTA would be a different message"""
    existing = tmp_path / "kept.tsv"
    existing.write_text("kept\n")
    cases = [["--pair-profile", existing, "missing.fa"], ["--pair-events", existing, "missing.fa"],
             ["--pair-profile", "p.tsv", "--pair-events", existing, "missing.fa"],
             ["--window", "100", "missing.fa"], ["--min-event", "10", "missing.fa"],
             ["--window", "100", "--pair-events", "e.tsv", "missing.fa"], ["--min-event", "10", "--pair-profile", "p.tsv", "missing.fa"],
             ["--pair-profile", "p.tsv", "-c", "missing.fa"], ["--pair-events", "e.tsv", "-c", "missing.fa"]]
    for bad in ("0", "-3", "1.5", "ten", "", "+4", "1e3"):
        cases.append(["--pair-profile", "p.tsv", "--window", bad, "missing.fa"])
        cases.append(["--pair-events", "e.tsv", "--min-event", bad, "missing.fa"])
    for args in cases:
        r = tps.run(args, tmp_path)
        assert tps.refused(r), (args, r.stderr)
        assert "missing.fa" not in r.stderr.decode(), args
        assert sorted(os.listdir(tmp_path)) == ["kept.tsv"], args
    assert existing.read_text() == "kept\n"
    # accepted: the run gets as far as the missing FASTA
    for args in (["--pair-profile", "p.tsv", "--window", "1"], ["--pair-events", "e.tsv", "--min-event", "1"], ["--pair-profile", "p.tsv", "--pair-events", "e.tsv"]):
        r = tps.run(["-v", "0"] + args + ["missing.fa"], tmp_path)
        assert tps.refused(r) and "missing.fa" in r.stderr.decode(), args
    assert sorted(os.listdir(tmp_path)) == ["kept.tsv"]


def test_cli_two_sequences_need_a_graph(tmp_path):
    """refused once the FASTA is read, before a device is opened: without --force-gfa-output two sequences print a CIGAR, no graph"""
    (tmp_path / "in.fa").write_text(">a\nACGTACGT\n>b\nACGAACGT\n")
    for args in (["--pair-profile", "p.tsv"], ["--pair-events", "e.tsv"]):
        r = tps.run(["-v", "0"] + args + ["in.fa"], tmp_path)
        assert tps.refused(r) and "--force-gfa-output" in r.stderr.decode(), args
    assert sorted(os.listdir(tmp_path)) == ["in.fa"]


def test_cli_new_options_are_not_parameters(tmp_path):
    base = tps.run(["-G"], tmp_path)
    got = tps.run(["--pair-profile", "p.tsv", "--window", "10", "--pair-events", "e.tsv", "--min-event", "3", "-G"], tmp_path)
    assert base.returncode == got.returncode == 0 and got.stdout == base.stdout and got.stderr == b""
    for word in (b"pair-profile", b"pair_profile", b"--window", b"pair-events", b"pair_events", b"min-event", b"min_event"):
        assert word not in got.stdout, word
    assert os.listdir(tmp_path) == []
    h = tps.run(["-h"], tmp_path)
    assert h.returncode == 0
    for opt in ("--pair-profile FILE", "--window INT", "--pair-events FILE", "--min-event INT"):
        assert opt in h.stderr.decode(), opt
