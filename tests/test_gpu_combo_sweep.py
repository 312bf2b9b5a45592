"""GPU suite: the sparse affine chaining DP across the number of chain combinations of a merge (pairs of paths that share a match pair).  cl_chain_device.cpp
changes its device path with that number — the one-combination specialisations, chain_walk2 up to 8, granules up to 16 and one atomic maximum + arrival count
per pair beyond, one / two / three combinations per walk workgroup up to 256 / 512 / 768, the group-by-group kernels beyond, parallel or serial numbering of the
combinations around 4 096 tags, several launches where a combination index is a launch dimension beyond 65 535 — and tests/helpers.py:combo_cases() has an
input on both sides of each of these counts, at one macro-block and (up to 1 056 combinations) at more than five.

Everything is bit-exact: DP values as uint32 patterns and the chain, against the chaining oracle — run here where it takes about 2 s at most, from
tests/golden/chain_combo_sweep.npz otherwise (tests/test_combo_sweep.py pins both to each other and to the compiled reference).  The path a DP took is read
from the library's own CL_CHAIN_TIMING lines in a child process per case (the switches are read once per process): a test that cannot show which path ran has
not tested the row."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = H.combo_cases()
NAMES = [c.name for c in CASES]
CHILD_TIMEOUT_S = 120
# every switch of the chaining DP a variant below may set, and the ones that would change a default path: cleared from a child's environment
SWITCHES = ("CL_CHAIN_FAR_MODE", "CL_CHAIN_NO_FAR_PRUNE", "CL_CHAIN_OLD_WALK", "CL_CHAIN_WALK_REDUCE", "CL_CHAIN_FAR_LANES", "CL_CHAIN_WALK2", "CL_CHAIN_WALK2_QPT",
            "CL_CHAIN_WALK2_HELPERS", "CL_CHAIN_WALK2_MAX", "CL_CHAIN_SEAL_WAVE", "CL_CHAIN_NEAR_SPLIT", "CL_CHAIN_EXT_EVENTS", "CL_CHAIN_LAZY_ACC", "CL_CHAIN_WALK_FOLD",
            "CL_CHAIN_DENSE_QUERIES", "CL_CHAIN_FAR_WAIT_LATE", "CL_CHAIN_GROUP_PATH", "CL_CHAIN_PAR_RECORDS_MIN", "CL_CHAIN_FAR_LAG", "CL_CHAIN_FAR_ARENA_SKIP",
            "CL_CHAIN_DEBUG_STALL", "CL_CHAIN_DEBUG_SKIP_FAR", "CL_CHAIN_WALK2_DEBUG", "CL_CHAIN_NO_SPARSE_INTRA")
_Z, _expected, _saved = {}, {}, {}


def golden():
    if "z" not in _Z:
        _Z["z"] = np.load(os.path.join(H.GOLDEN, "chain_combo_sweep.npz"))
    return _Z["z"]


def expected(case, glob=True):
    """(DP bit patterns, chain) of the oracle: computed once per case and anchoring, shared by every test, never changed"""
    key = (case.name, glob)
    if key not in _expected:
        g1, g2, ms, scale = H.combo_input(case)
        if H.combo_oracle_is_live(case):
            chain, dp = po.oracle_chain("affine", g1, g2, ms, scale=scale, want_dp=True, global_anchoring=glob)
            _expected[key] = (dp[:ms.n_pairs()].view(np.uint32).copy(), chain)
        else:
            pre = "%s/%s/" % (case.name, "global" if glob else "local")
            _expected[key] = (golden()[pre + "dp"], golden()[pre + "chain"])
        for a in _expected[key]:
            a.setflags(write=False)
    return _expected[key]


def expected_digests(case):
    g1, g2, ms, scale = H.combo_input(case)
    dp, chain = expected(case)
    return (str(ms.n_pairs()), str(len(chain))) + far_ab_child.digests(dp.view(np.float32), np.ascontiguousarray(chain, np.uint32))


@pytest.fixture(scope="module")
def input_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("combo_sweep")


def saved_input(case, input_dir):
    if case.name not in _saved:
        path = str(input_dir / (case.name + ".npz"))
        far_ab_child.save_input(path, *H.combo_input(case))
        _saved[case.name] = path
    return _saved[case.name]


class Run:
    """what one child process reported: the RESULT digests and the paths named by the library's timing lines"""

    def __init__(self, stdout, stderr):
        m = re.search(r"RESULT pairs=(\d+) anchors=(\d+) dp=(\w+) chain=(\w+)", stdout)
        assert m, stdout[-2000:] + stderr[-3000:]
        self.result, self.err = m.groups(), stderr
        # (a DP whose walk had to be repeated logs its lines once per attempt: the last ones are those of the values returned)
        self.pairs, self.combos, self.records = [int(x) for x in re.findall(r"\[chain_dp_batch\]\s+(\d+) pairs, (\d+) combinations, (\d+) records", stderr)[-1]]
        self.queries, self.far, t1, t2, self.walk = re.findall(r"device memory held by the context: [\d.]+ MB \((\w+) queries, far pass (\w+):.* (\d+) \+ (\d+) tags, walk (\w+)\)", stderr)[-1]
        self.tags = int(t1) * int(t2)      # (a tag per chain of the path merge: one more than paths on either side)
        m = re.findall(r"\[chain_dp_batch\]\s+path: ([\w-]+), exchange ([\w+]+), fold (\d+), helpers (\d+), numbering (\w+), arrays (\w+), far (\w+)", stderr)[-1]
        self.path, self.exchange, self.fold, self.helpers, self.numbering, self.arrays, self.far_mode = m[0], m[1], int(m[2]), int(m[3]), m[4], m[5], m[6]
        self.rows = re.findall(r"\[chain_dp_batch\]\s+traceback rows ([\w ]+)\n", stderr)[-1]


def run_child(case, input_dir, env_extra=None):
    """one DP in a process of its own under CL_CHAIN_TIMING=1, every other switch cleared; no retry: a child that fails or runs out of time fails the test there"""
    env = dict(os.environ, CL_CHAIN_TIMING="1")
    for k in SWITCHES:
        env.pop(k, None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "far_ab_child.py"), saved_input(case, input_dir), "affine"], env=env, capture_output=True, text=True,
                       timeout=CHILD_TIMEOUT_S)
    assert r.returncode == 0, (case.name, env_extra, r.stdout[-2000:] + r.stderr[-3000:])
    return Run(r.stdout, r.stderr)


def expected_records(case):
    """records of a case, counted from its inputs"""
    return H.count_records(*H.combo_input(case)[:3])


def expected_arrays(case):
    """a DP is packed into one device block up to 2 MB: per pair and combination a query (12 B), an own-record slot (4 B) and seven results (28 B), per record four
    fields and seven values (44 B), and some small change.  No case is nearer to the limit than 2 x 2 paths at 5 200 pairs (1.8 MB)"""
    return "separate" if 44 * (H.combo_input(case)[2].n_pairs() * case.combos + expected_records(case)) > 2 << 20 else "packed"


WALK2_HELPERS = 7      # chain_walk2's main workgroup keeps a window of 128 queries of the macro-block's 1 024: a helper for each of the other seven sub-blocks


def default_path(case):
    """the path the table of thresholds gives for the case (walk field, path, exchange, fold), from its number of combinations and — for chain_walk2, which is for
    DPs too large to be packed into one block — from its size"""
    n = case.combos
    if n > 3 * 256:
        return ("off", "groups", "none", 0)
    fold = (n + 255) // 256
    if fold > 1:
        return ("fold", "walk", "reduce", fold)
    if n <= 8 and expected_arrays(case) == "separate":
        return ("2", "walk", "none" if n == 1 else "walk2", 1)
    return ("1", "walk", "none" if n == 1 else "reduce" if n > 16 else "granules", 1)


# (a) the default path, in process ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_dp_values_and_chain_are_the_oracles(gpu_ctx, name):
    """every case on the default path: DP bit patterns and chain, under global anchoring and — one macro-block and less — under local anchoring.
    The three counts around 65 535 (255 x 257, 256 x 256, 256 x 257 paths) are cases like any other: such a DP must work, not be refused.  They run group by group,
    with the combination index in grid.y of chain_expand_queries_kernel and grid.z of chain_group_push_kernel; 65 792 combinations take two launches of each
    (kChainGridCombos).  Measured on an MI355X before the launches were split: the runtime accepted 65 536 and 65 792 in grid.y and grid.z, and the DP values and chain
    at 65 535, 65 536 and 65 792 combinations were already these: the split keeps the launches inside the documented limit, it repairs nothing that was seen to fail."""
    case = H.combo_case(name)
    g1, g2, ms, scale = H.combo_input(case)
    for glob in ((True,) if case.size == "multi" else (True, False)):
        dp, chain = expected(case, glob)
        got = gpu_ctx.chain_sparse_affine(g1, g2, ms, scale=scale, want_dp=True, params=capi.default_chain_params(global_anchoring=glob))
        assert len(got["dp"]) == ms.n_pairs() == len(dp)
        diff = np.flatnonzero(got["dp"].view(np.uint32) != dp)
        assert len(diff) == 0, "%s, %s anchoring: %d of %d DP values differ, first at pair %d" % (name, "global" if glob else "local", len(diff), len(dp), diff[0])
        assert np.array_equal(got["chain"], chain), (name, glob)


# (b) which path ran ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_default_path_is_the_one_the_combination_count_selects(input_dir, name):
    case = H.combo_case(name)
    run = run_child(case, input_dir)
    print(name, run.result, run.pairs, run.combos, run.queries, run.far, run.walk, run.path, run.exchange, run.fold, run.helpers, run.numbering, run.arrays, run.rows)
    assert run.result == expected_digests(case), name
    assert run.combos == case.combos == H.count_combinations(*H.combo_input(case)[:3])
    assert (run.walk, run.path, run.exchange, run.fold) == default_path(case), name
    assert run.arrays == expected_arrays(case)
    assert run.helpers == (WALK2_HELPERS if run.walk == "2" else 0)
    ms = H.combo_input(case)[2]
    assert run.pairs == ms.n_pairs()
    assert run.queries == ("factored" if case.combos * ms.n_pairs() > 100000 else "dense")
    # (the parallel numbering is for 2^20 records and more — the multi-block cases from 256 combinations on — and 4 096 tags at most;
    # test_numbering_and_query_table_variants asks for it at every size)
    assert run.tags == (case.p1 + 1) * (case.p2 + 1)
    assert run.records == expected_records(case)
    assert run.numbering == ("parallel" if expected_records(case) >= 1 << 20 and run.tags <= 4096 else "serial")
    assert run.rows == "downloaded"
    if ms.n_pairs() > 1024:
        # five macro-blocks and more: the far pass runs wherever the walk does, and from 8 combinations on the arrays are too large to be packed (chain_walk2's condition)
        assert run.pairs > 4 * 1024
        assert run.far == ("on" if case.combos <= 768 else "off")
        assert run.far_mode == ("bb" if case.combos <= 768 else "none")      # (too few macro-blocks for a checkpoint: the branch-and-bound throughout)
        assert case.combos < 8 or expected_arrays(case) == "separate"
    else:
        assert run.pairs <= 1024 and run.far == "off" and run.far_mode == "none"


def check_variants(case, input_dir, variants):
    """every variant in a child of its own: the digests of the expected values, and what the variant's check says about the path"""
    want = expected_digests(case)
    assert len(variants) <= 6
    for env, check in variants:
        run = run_child(case, input_dir, env)
        assert run.result == want, (case.name, env)
        assert run.combos == case.combos
        check(run)


# (c) the variants at the thresholds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1_multi", "1x2_multi"])
def test_per_block_kernels_around_one_combination(input_dir, name):
    """one combination: chain_intra_kernel's `simple` walk with the near pass folded in; two: the general one with near launches in front of it"""
    def per_block(run):
        assert (run.walk, run.path) == ("off", "per-block")
    check_variants(H.combo_case(name), input_dir, [({"CL_CHAIN_OLD_WALK": "1", "CL_CHAIN_NO_FAR_PRUNE": "1"}, per_block)])


@pytest.mark.parametrize("name", ["2x4_multi", "3x3_multi"])
def test_walk2_variants_around_8_combinations(input_dir, name):
    def walk1(run):
        assert run.walk == "1" and run.exchange == "granules"
    def helpers(n):
        def check(run):
            assert run.walk == "2" and run.helpers == n
        return check
    check_variants(H.combo_case(name), input_dir, [({"CL_CHAIN_WALK2": "0"}, walk1), ({"CL_CHAIN_WALK2_HELPERS": "0", "CL_CHAIN_WALK2_MAX": "9"}, helpers(0)),
                                                   ({"CL_CHAIN_WALK2_HELPERS": "2", "CL_CHAIN_WALK2_MAX": "9"}, helpers(2))])


@pytest.mark.parametrize("name", ["4x4_multi", "1x17_multi", "2x9_multi", "4x4_small", "1x17_small", "2x9_small"])
def test_exchange_variants_around_16_combinations(input_dir, name):
    def exchange(kind):
        def check(run):
            assert run.walk == "1" and run.exchange == kind
        return check
    check_variants(H.combo_case(name), input_dir, [({"CL_CHAIN_WALK_REDUCE": "0"}, exchange("granules")), ({"CL_CHAIN_WALK_REDUCE": "1"}, exchange("reduce"))])


@pytest.mark.parametrize("name", ["16x16_multi", "1x257_multi", "16x16_small", "1x257_small"])
def test_fold_variants_around_256_combinations(input_dir, name):
    def fold(n):
        def check(run):
            assert run.walk == "fold" and run.fold == n and run.exchange == "reduce"
        return check
    check_variants(H.combo_case(name), input_dir, [({"CL_CHAIN_WALK_FOLD": "2"}, fold(2)), ({"CL_CHAIN_WALK_FOLD": "3"}, fold(3))])


@pytest.mark.parametrize("name", ["24x32_small", "22x35_small", "32x33_small"])
def test_per_block_and_group_variants_around_768_combinations(input_dir, name):
    case = H.combo_case(name)
    def no_groups(run):       # (768 combinations are the walk's, three per workgroup, whatever this switch says)
        assert (run.walk, run.path) == (("fold", "walk") if case.combos <= 768 else ("off", "per-block"))
    def per_block(run):
        assert (run.walk, run.path) == ("off", "per-block")
    def groups(run):
        assert (run.walk, run.path) == ("off", "groups")
    variants = [({"CL_CHAIN_GROUP_PATH": "0"}, no_groups), ({"CL_CHAIN_OLD_WALK": "1", "CL_CHAIN_NO_FAR_PRUNE": "1"}, per_block)]
    if case.combos == 1056:
        variants.append(({"CL_CHAIN_GROUP_PATH": "force"}, groups))
    check_variants(case, input_dir, variants)


@pytest.mark.parametrize("name", ["4x4_disjoint", "1x17_disjoint", "16x16_disjoint"])
def test_every_combination_counts_where_paths_share_no_node(input_dir, name):
    """over graphs whose paths share no node a match pair lies in one combination and has its predecessors there alone: a combination left out — the last granule of
    the sweep, an arrival count one short, the last combination of a partly filled workgroup of the fold (16 = 5 x 3 + 1, 17 = 8 x 2 + 1, 256 = 85 x 3 + 1), the last grid.z of the
    group path's push — changes DP values.  Both exchanges, both folds and the group-by-group path on 16, 17 and 256 combinations.
    Not caught here or anywhere: an arrival count compared with one workgroup too few.  The workgroups of a pair arrive within the time the first needs to see its own
    arrival come back, so the late candidate was in place in every run of that mutation (nine tests, 16 to 256 workgroups); showing it needs a workgroup held back
    on purpose, which nothing in the library can do."""
    def exchange(kind):
        def check(run):
            assert run.walk == "1" and run.exchange == kind
        return check
    def fold(n):
        def check(run):
            assert run.walk == "fold" and run.fold == n
        return check
    def groups(run):
        assert (run.walk, run.path) == ("off", "groups")
    check_variants(H.combo_case(name), input_dir, [({"CL_CHAIN_WALK_REDUCE": "0"}, exchange("granules")), ({"CL_CHAIN_WALK_REDUCE": "1"}, exchange("reduce")),
                                                   ({"CL_CHAIN_WALK_FOLD": "2"}, fold(2)), ({"CL_CHAIN_WALK_FOLD": "3"}, fold(3)), ({"CL_CHAIN_GROUP_PATH": "force"}, groups)])


def test_per_block_launches_beyond_65535_combinations(input_dir):
    """the per-block kernels put the combination index into grid.z of chain_inter_kernel: at 65 792 combinations its second launch starts at combination 65 535"""
    def per_block(run):
        assert (run.walk, run.path) == ("off", "per-block")
    check_variants(H.combo_case("256x257_tiny"), input_dir, [({"CL_CHAIN_GROUP_PATH": "0"}, per_block)])


def test_far_modes_on_a_multi_block_case(input_dir):
    def bb(run):
        assert run.far == "on" and run.far_mode == "bb"
    def sweep(run):
        assert run.far == "on" and run.far_mode == "sweep"
    check_variants(H.combo_case("2x9_multi"), input_dir, [({"CL_CHAIN_FAR_MODE": "bb"}, bb), ({"CL_CHAIN_FAR_MODE": "sweep"}, sweep)])


@pytest.mark.parametrize("name", ["32x33_multi", "64x64_small", "64x65_small"])
def test_numbering_and_query_table_variants(input_dir, name):
    """traceback rows on demand, dense query tables, and the parallel numbering of the combinations asked for at every size: it is for 4 096 tags at most, and a
    side has one tag more than paths: 33 x 34 = 1 122 tags number in parallel, 65 x 65 = 4 225 and 65 x 66 = 4 290 serially"""
    case = H.combo_case(name)
    def lazy(run):
        assert run.rows == "on demand"
    def dense(run):
        assert run.queries == "dense"
    def numbering(run):
        assert run.tags == (case.p1 + 1) * (case.p2 + 1) and run.numbering == ("parallel" if run.tags <= 4096 else "serial")
    check_variants(case, input_dir, [({"CL_CHAIN_LAZY_ACC": "1"}, lazy), ({"CL_CHAIN_DENSE_QUERIES": "1"}, dense), ({"CL_CHAIN_PAR_RECORDS_MIN": "0"}, numbering)])
