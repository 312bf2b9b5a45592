"""GPU suite: the chaining DP (sparse_affine_chain_dp and the gap-free sparse_chain_dp) across the number of match pairs.  The driver and its kernels change what
they do with that number — a last block of kChainBlock = 256 pairs that is partial or holds one pair; a walk launch whose count is partial or 1 (kChainMacro = 1 024);
the first near launch and the first wait on ev_walk[k - 2]; the far pass on from lag + 3 macro-blocks, with exactly two far launches and two seals at its first
count; the levels of the far pass's node tree at 512, 4 096 and 32 768 records of the largest combination, and a second top-level node beyond; far_seal_big_kernel
from levels >= 2 on; one packed device block or separate arrays (and chain_walk2 with them); dense or factored query tables; no pair at all — and
tests/helpers.py:pair_cases() has an input on both sides of each count, in three families (tests/test_pair_sweep.py pins the inputs and what they must select).

Everything is bit-exact against the chaining oracle, run live: DP values as uint32 patterns and the chain.  Which path a DP took is read from the library's own
CL_CHAIN_TIMING lines.  The switches are read once per process, so every setting runs in ONE child process (tests/pair_sweep_child.py) over a list of cases; a child
is never run twice."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from centrolign_amd import capi
from oracle import pyoracle as po
from tests import far_ab_child
from tests import helpers as H
from tests.test_gpu_combo_sweep import SWITCHES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = H.pair_cases()
NAMES = [c.name for c in CASES]
ALGOS = ("affine", "sparse")
_expected, _saved, _children = {}, {}, {}


def expected(case, algo="affine", glob=True):
    """(DP bit patterns, chain) of the oracle: computed once per case, DP and anchoring, shared by every test, never changed.  (The oracle pads its DP array to
    length 1 where there is no pair: the slice below is empty there, and the tests compare lengths with the library's own count.)"""
    key = (case.name, algo, glob)
    if key not in _expected:
        g1, g2, ms, scale = H.pair_input(case)
        chain, dp = po.oracle_chain(algo, g1, g2, ms, scale=scale, want_dp=True, global_anchoring=glob)
        _expected[key] = (dp[:case.n].view(np.uint32).copy(), np.ascontiguousarray(chain, np.uint32))
        for a in _expected[key]:
            a.setflags(write=False)
    return _expected[key]


def expected_result(case, algo):
    dp, chain = expected(case, algo)
    return (case.n, len(chain)) + far_ab_child.digests(dp.view(np.float32), chain)


# (a) values, in process, default path -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_dp_values_and_chain_are_the_oracles(gpu_ctx, name):
    """the affine and the gap-free DP of every case under global anchoring and, up to 5 121 pairs, under local anchoring"""
    case = H.pair_case(name)
    g1, g2, ms, scale = H.pair_input(case)
    for algo in ALGOS:
        for glob in ((True, False) if case.n <= H.PAIR_LOCAL_MAX else (True,)):
            dp, chain = expected(case, algo, glob)
            got = gpu_ctx.chain_sparse_affine(g1, g2, ms, scale=scale, want_dp=True, sparse=algo == "sparse", params=capi.default_chain_params(global_anchoring=glob))
            what = "%s, %s, %s anchoring" % (name, algo, "global" if glob else "local")
            assert got["n_pairs"] == case.n == len(dp), what
            if case.n == 0:
                assert got["dp"] is None and len(got["chain"]) == 0 and len(chain) == 0, what
                continue
            assert len(got["dp"]) == case.n, what
            diff = np.flatnonzero(got["dp"].view(np.uint32) != dp)
            assert len(diff) == 0, "%s: %d of %d DP values differ, first at pair %d (macro-block %d, block %d)" % (what, len(diff), len(dp), diff[0], diff[0] // 1024, diff[0] // 256)
            assert np.array_equal(got["chain"], chain), what


# the children -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def input_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("pair_sweep")


def saved_input(case, input_dir):
    """the case's input with the oracle's DP values of both DPs beside it (the child counts the values that differ)"""
    if case.name not in _saved:
        path = str(input_dir / (case.name + ".npz"))
        far_ab_child.save_input(path, *H.pair_input(case), extra={"want." + algo: expected(case, algo)[0] for algo in ALGOS})
        _saved[case.name] = path
    return _saved[case.name]


class Run:
    """what a child reported of one DP: its RESULT line and the paths named by the library's timing lines behind its CASE line"""

    def __init__(self, result, err):
        self.result = (int(result[0]), int(result[1]), result[2], result[3])
        self.changed, self.err = int(result[4]), err
        self.logged = "[chain_dp_batch]" in err
        if not self.logged:
            return
        # (a DP whose walk had to be repeated logs its lines once per attempt: the last ones are those of the values returned)
        self.pairs, self.combos, self.records, self.largest = [int(x) for x in re.findall(r"(\d+) pairs, (\d+) combinations, (\d+) records \(largest combination (\d+)\)", err)[-1]]
        m = re.findall(r"\((\w+) queries, far pass (\w+): (\d+) padded records in (\d+) levels, \d+ \+ \d+ tags, walk (\w+)\)", err)[-1]
        self.queries, self.far, self.padded, self.levels, self.walk = m[0], m[1], int(m[2]), int(m[3]), m[4]
        m = re.findall(r"path: ([\w-]+), exchange ([\w+]+), fold (\d+), helpers (\d+), numbering (\w+), arrays (\w+), far (\w+)", err)[-1]
        self.path, self.exchange, self.arrays, self.far_mode = m[0], m[1], m[5], m[6]


def run_child(key, cases, input_dir, env_extra=None):
    """one process under CL_CHAIN_TIMING=1 for the whole list, every other switch cleared, a time limit sized to the list (a context, then some tens of
    milliseconds per DP: 60 s and 2 s per case are generous).  Run once per key: a child that failed fails every test that needs it, and is not started again"""
    if key not in _children:
        env = dict(os.environ, CL_CHAIN_TIMING="1")
        for k in SWITCHES:
            env.pop(k, None)
        env.update(env_extra or {})
        args = ["%s=%s" % (c.name, saved_input(c, input_dir)) for c in cases]
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pair_sweep_child.py")] + args, env=env, capture_output=True, text=True, timeout=60 + 2 * len(cases))
            assert r.returncode == 0, (key, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
            results = {(m[0], m[1]): m[2:] for m in re.findall(r"RESULT case=(\w+) algo=(\w+) pairs=(\d+) anchors=(\d+) dp=(\w+) chain=(\w+) changed=(-?\d+)", r.stdout)}
            parts = re.split(r"^CASE (\w+) (\w+)\n", r.stderr, flags=re.M)
            logs = {(parts[i], parts[i + 1]): parts[i + 2] for i in range(1, len(parts) - 2, 3)}
            assert set(results) == set(logs) == {(c.name, a) for c in cases for a in ALGOS}, (key, r.stdout[-2000:] + r.stderr[-3000:])
            _children[key] = {k: Run(results[k], logs[k]) for k in results}
        except Exception as e:      # (an assertion above, or the time limit)
            _children[key] = e
    if isinstance(_children[key], Exception):
        raise AssertionError("child %s failed: %r" % (key, _children[key]))
    return _children[key]


def check_values(runs, case, what):
    """both DPs of a case in a child: the digests of the expected values; the first differing pair is what the child's count and test (a) are for"""
    for algo in ALGOS:
        run = runs[(case.name, algo)]
        assert run.result == expected_result(case, algo), "%s %s %s: %d DP values differ from the oracle's" % (what, case.name, algo, run.changed)
        assert run.changed == 0


def default_path(pred):
    """(walk, path, exchange) of the default switches: chain_walk2 wherever the arrays are separate and there are at most 8 combinations"""
    return (pred.walk, "walk", "none" if pred.combos == 1 else "walk2" if pred.walk == "2" else "granules")


# (b) which path ran --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_default_path_is_the_one_the_pair_count_selects(input_dir, name):
    """one child per family at default switches.  From the library's own lines: pairs, combinations, records and the largest combination; the far pass on from five
    macro-blocks; the padded records and the levels of its node tree; packed or separate arrays on both sides of the mirrored PackLayout's 2 MB; chain_walk2 exactly
    where the arrays are separate and there are at most 8 combinations; factored queries exactly beyond 100 000 combinations x pairs.
    The gap-free DP files a pair under the first chain of each end only: its records are the pairs, and its combinations are the affine DP's wherever every end
    node lies on one path (families A and C), so that everything but the exchange is asserted for it there too."""
    case = H.pair_case(name)
    pred = H.pair_prediction(case)
    runs = run_child("default_" + case.family, H.pair_cases(case.family), input_dir)
    check_values(runs, case, "default")
    for algo in ALGOS:
        run = runs[(name, algo)]
        if case.n == 0:      # nothing to do: the driver returns before it logs anything
            assert not run.logged and run.result[:2] == (0, 0)
            continue
        print(name, algo, run.pairs, run.combos, run.records, run.largest, run.queries, run.far, run.padded, run.levels, run.walk, run.path, run.exchange, run.arrays, run.far_mode)
        assert run.pairs == case.n
        assert run.far == ("on" if (case.n + 1023) // 1024 >= 5 else "off") == ("on" if pred.far else "off")
        assert run.far_mode == ("bb" if pred.far else "none")
        assert run.path == "walk"
        if algo == "sparse" and case.family == "B":
            assert run.records == case.n and 1 <= run.combos <= 4
            continue
        assert (run.combos, run.records, run.largest) == (pred.combos, pred.records, pred.largest)
        assert (run.padded, run.levels) == ((pred.padded, pred.levels) if pred.far else (0, 0))
        assert run.arrays == ("packed" if pred.packed else "separate")
        assert run.walk == ("2" if run.arrays == "separate" and run.combos <= 8 else "1") == pred.walk
        assert run.queries == ("factored" if run.combos * run.pairs > 100000 else "dense")
        if algo == "affine":
            assert (run.walk, run.path, run.exchange) == default_path(pred)


# (c) the switches at the edges -----------------------------------------------------------------------------------------------------------------------------
def edge_cases(families):
    return [c for c in CASES if c.family in families and c.n in H.PAIR_EDGE_LIST]


def is_per_block(run, pred):
    assert (run.walk, run.path, run.far, run.far_mode) == ("off", "per-block", "off", "none")


def is_groups(run, pred):
    assert (run.walk, run.path, run.far) == ("off", "groups", "off")


def far_mode(mode):
    def check(run, pred):
        assert run.path == "walk" and (run.far, run.far_mode) == (("on", mode) if pred.far else ("off", "none"))
    return check


def is_default(run, pred):
    """(CL_CHAIN_NEAR_SPLIT, CL_CHAIN_FAR_WAIT_LATE and CL_CHAIN_EXT_EVENTS change the order of launches and events and leave no mark in the log: the path must
    still be the walk's, with the far pass wherever the default has it)"""
    assert run.path == "walk" and (run.far, run.far_mode) == (("on", "bb") if pred.far else ("off", "none"))


def is_reduce(run, pred):
    assert run.path == "walk" and run.exchange == ("none" if run.combos == 1 else "walk2+reduce" if run.walk == "2" else "reduce")


SETTINGS = {
    "per_block": ({"CL_CHAIN_OLD_WALK": "1", "CL_CHAIN_NO_FAR_PRUNE": "1"}, "ABC", is_per_block),
    "groups": ({"CL_CHAIN_GROUP_PATH": "force"}, "BC", is_groups),
    "sweep": ({"CL_CHAIN_FAR_MODE": "sweep"}, "ABC", far_mode("sweep")),
    "bb_seal_by_waves": ({"CL_CHAIN_FAR_MODE": "bb", "CL_CHAIN_SEAL_WAVE": "1"}, "ABC", far_mode("bb")),
    "near_in_two_launches": ({"CL_CHAIN_NEAR_SPLIT": "1"}, "ABC", is_default),
    "far_sent_at_its_own_block": ({"CL_CHAIN_FAR_WAIT_LATE": "1"}, "ABC", is_default),
    "event_records": ({"CL_CHAIN_EXT_EVENTS": "0"}, "ABC", is_default),
    "reduce": ({"CL_CHAIN_WALK_REDUCE": "1"}, "BC", is_reduce),
}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_switches_at_the_edges(input_dir, setting):
    """every scheduling and path variant where k - 2 and k - lag - 1 are 0, where a launch's count is 1 and where the last block holds one pair: the edge list of
    every family in one child per setting"""
    env, families, check = SETTINGS[setting]
    cases = edge_cases(families)
    assert len(cases) == len(families) * len(H.PAIR_EDGE_LIST)
    runs = run_child(setting, cases, input_dir, env)
    for case in cases:
        check_values(runs, case, setting)
        pred = H.pair_prediction(case)
        for algo in ALGOS:
            run = runs[(case.name, algo)]
            assert run.pairs == case.n
            check(run, pred)
            print(setting, case.name, algo, run.path, run.walk, run.exchange, run.far, run.far_mode)


@pytest.mark.parametrize("lag", H.PAIR_FAR_LAGS)
def test_far_lag_moves_the_far_pass(input_dir, lag):
    """CL_CHAIN_FAR_LAG = 1, 3, 8 (kFarLag): the far pass is off at lag + 2 macro-blocks and on at one pair more, where far(lag + 2) — one query — waits for seal(0)"""
    edge = (lag + 2) * 1024
    cases = [H.pair_case("%s_%d" % (fam, n)) for fam in "AC" for n in (edge, edge + 1)]
    runs = run_child("lag%d" % lag, cases, input_dir, {"CL_CHAIN_FAR_LAG": str(lag)})
    for case in cases:
        check_values(runs, case, "lag %d" % lag)
        for algo in ALGOS:
            run = runs[(case.name, algo)]
            assert run.pairs == case.n and run.path == "walk"
            assert (run.far, run.far_mode) == (("off", "none") if case.n == edge else ("on", "bb")), (case.name, algo)


# (d) the far pass must matter in these inputs ---------------------------------------------------------------------------------------------------------------
def test_dp_values_depend_on_the_far_launches(input_dir):
    """a far pass that found nothing would pass everything above if the near range always held the best predecessor.  CL_CHAIN_DEBUG_SKIP_FAR=1 leaves the far
    launches out and nothing else (documented as giving wrong results): on the far-on cases listed in helpers.PAIR_SKIP_FAR the values of both DPs must then differ
    from the oracle's, so in these inputs some pair takes its predecessor from more than two macro-blocks back.  The counts measured on an MI355X stand beside
    PAIR_SKIP_FAR in tests/helpers.py."""
    cases = [H.pair_case("%s_%d" % (fam, n)) for fam in sorted(H.PAIR_SKIP_FAR) for n in H.PAIR_SKIP_FAR[fam]]
    runs = run_child("skip_far", cases, input_dir, {"CL_CHAIN_DEBUG_SKIP_FAR": "1"})
    for case in cases:
        for algo in ALGOS:
            run = runs[(case.name, algo)]
            print("without the far launches: %s %s: %d of %d DP values changed" % (case.name, algo, run.changed, case.n))
            assert run.pairs == case.n and run.far == "on" and run.result[0] == case.n
    for case in cases:
        for algo in ALGOS:
            run = runs[(case.name, algo)]
            assert run.changed > 0 and run.result[2] != expected_result(case, algo)[2], (case.name, algo)
