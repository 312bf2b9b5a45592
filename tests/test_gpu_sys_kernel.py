"""The systolic DAG kernel of the stitch path, popoa_sys_kernel<NPW, BLOCK> (sys_sweep in popoa_kernels.hip), in every instantiation, ring depth, LDS class and
saved-column mode, bit for bit against the oracle.

It is the default route of every branching pair whose shorter side fits one workgroup.  CL_NO_LANE=1 (read per plan) keeps the near-chain shapes among the ones here
away from the register kernel; the group of one-node pairs also sets CL_FORCE_GENERAL=1, which sends chain pairs (1 x 1 is always one) past the chain kernels.  Every
plan holds fewer than 2 048 subproblems, so the narrow launch does not absorb the launches.  Every plan is checked against choose_sys's rule as tests/test_sys_rule.py
restates it from the batch alone (that file asserts, without a device, that the restatement is the packer's and that every shape below is in the class it was built
for): the popoa_sys_kernel launches are exactly the ones the rule predicts — instantiation, number of pairs, their cells, dynamic LDS (the largest footprint of the
members) — so the pairs the rule takes ran on this kernel and on nothing else.  The pairs it refuses ride along on whatever takes them and are compared as well.

What the shapes are for (tests/test_sys_rule.py builds them):
  * workgroup sizes 64 / 256 / 1 024 for a shorter side + 1 of <= 64 / <= 256 / above: shorter sides 63 | 64, 127 | 128, 255 | 256 in both orientations; the most rows
    the rule takes at each NumPW and one more; pairs of one node.  The 128-thread instantiations exist only under CL_SYS_BLOCK128=1, read once per process: one child;
  * ring depths: for each candidate near limit a column graph with a skip of exactly that many columns (2 047 fills the record's 11-bit field) and one of one more,
    which is saved; every log2 H from 2 to 12; more than 2 H columns wherever 159 KB allow it, so that the rings wrap;
  * saved columns: 1, 2, 32 and (refused at that limit) 33 of them; the far predecessor first and last in a column's list (the straight-line cell's f0 != f1 both
    ways); a saved column read from 1, 2 and 200 columns on, itself a fork; column 0 saved for a late source, alone and with others, and not saved for an early one;
    synth.far_fork_batch at sizes the rule takes;
  * cells: in-degrees 1, 2, 3, sources with one and two predecessors and without any in mid-graph, on both sides (all four of fastR x fastC), under the packer's
    rank order and the reference's; a column with 63 predecessors (64: refused), a row with 64; the leading-gap and two-gaps pairs of tests/test_gpu_general_kernels.py,
    which decide boundary and source terms that random inputs leave undecided;
  * every (NumPW, BLOCK) with at most 64 KB and with more of dynamic LDS; a mixed batch whose LDS classes share a launch; a resident plan executed three times.

That the tests bite was checked in scratch builds with one thing of sys_sweep changed each (every access still inside the workgroup's LDS and planes):
  * pred_code with >= for > (where the pair has saved columns): edges_dags and others fail;
  * no corner term `if (srcR) M = imax(M, s)`: cells (ties) and degenerate fail;
  * a missing second column predecessor repeating the boundary instead of the first (where the pair has saved columns): cells fails;
  * save_col0 ignored: cells fails (saved_columns holds the late sources built for it);
  * no source term of V in the interior: random_dags under `pieces` fails, and nothing else — the one thin spot;
  * where() with <= for <: passes, and cannot but pass.  A read at exactly H columns behind the row's position finds the ring slot still holding that column: the
    row overwrites it in this very step, after its reads, and a wave's reads of a step precede its writes.  Across the waves of a workgroup it is a race;
  * the boundary row's M' given the value of M: passes, and cannot but pass under an admissible scoring.  Only the boundary row reads its own M'; what changes is its
    H_k for the pieces k that are not the cheapest at that length, to a value that still stays below the row's M (a gap's cost is concave in its length: opening
    another piece in mid-gap never pays), so neither a score nor the traceback's equality tests see it.

What this file cannot show: the barrier.  At BLOCK > 64 the waves of a workgroup meet at an LDS-only barrier after every step; a sweep whose barrier were weakened is a
race that may still give the oracle's bytes on every run, and no test here claims to catch it."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from centrolign_amd import capi
from oracle import pyoracle as po
from tests import test_sys_rule as R
from tests.test_gpu_general_kernels import _params, _same_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_NAMES = ("CL_FORCE_GENERAL", "CL_NO_SYS", "CL_NO_RING", "CL_NO_STRIP", "CL_NO_LANE", "CL_RANK_ORDER", "CL_LANE_MIN_SWEEP", "CL_STITCH_LDS_CLASSES")
_oracle = {}
_seen = {}       # (group, order, NumPW) -> the popoa_sys_kernel launches of the group's plan, from test_against_the_oracle where that ran first


def _set_hooks(monkeypatch, group, order):
    for name in HOOK_NAMES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("CL_NO_LANE", "1")
    if group in R.FORCE_GENERAL:
        monkeypatch.setenv("CL_FORCE_GENERAL", "1")
    if order != "auto":
        monkeypatch.setenv("CL_RANK_ORDER", order)


def _want(group, batch, npw, which):
    """the oracle's result does not depend on the rank order"""
    key = (group, npw, which)
    if key not in _oracle:
        _oracle[key] = po.oracle_stitch_batch(batch, params=_params(which), force_num_pw=np.full(batch.n_problems, npw, np.uint8))
    return _oracle[key]


def _cells(batch, pairs):
    n1, n2 = batch.sizes()
    return int(sum((int(n1[k]) + 1) * (int(n2[k]) + 1) for k in pairs))


def sys_launches(plan):
    """(kernel, pairs, dynamic LDS) of the plan's popoa_sys_kernel launches, sorted; the cells of all of them"""
    out, cells = [], 0
    for li in plan.launches():
        if li["n_problems"] and li["kernel"].startswith(R.SYS):
            assert re.fullmatch(r"popoa_sys_kernel<[123], (64|128|256|1024)>", li["kernel"]), li["kernel"]
            out.append((li["kernel"], li["n_problems"], li["lds_bytes"]))
            cells += li["dp_cells"]
    return sorted(out), cells


def _plan(gpu_ctx, monkeypatch, group, batch, npw, params=None, order="auto"):
    """a plan of the batch, its popoa_sys_kernel launches checked against the rule"""
    _set_hooks(monkeypatch, group, order)
    plan = gpu_ctx.plan(batch, params=params, force_num_pw=npw)
    want, taken = R.predicted_launches(batch, npw, order, force_general=group in R.FORCE_GENERAL)
    got, cells = sys_launches(plan)
    assert got == want and cells == _cells(batch, taken), "%s: the plan's launches %r (%d cells) are not what choose_sys's rule predicts, %r (%d cells)" % (group, got, cells, want, _cells(batch, taken))
    return plan, got


# ---- every group against the oracle, every NumPW, three scorings ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", ["default", "ties", "pieces"])
@pytest.mark.parametrize("group,order", R.runs())
def test_against_the_oracle(gpu_ctx, monkeypatch, group, order, scoring):
    b = R.batch_of(group)
    for npw in (1, 2, 3):
        want = _want(group, b, npw, scoring)
        plan, launches = _plan(gpu_ctx, monkeypatch, group, b, np.full(b.n_problems, npw, np.uint8), _params(scoring), order)
        plan.execute(); plan.sync()
        diff = plan.collect().same_as(want)
        plan.destroy()
        assert diff is None, "%s, %s order, NumPW %d, %s scores: %s" % (group, order, npw, scoring, diff)
        _seen[(group, order, npw)] = launches


# ---- the 128-thread instantiations ---------------------------------------------------------------------------------------------------------------------------
def _block128_batch(which):
    """65 to 128 rows with the boundary row.  "small": 65 rows of a random DAG and 101 of a chain, at most 64 KB each; "large": the random pairs of 64 and 127
    nodes and the pairs of 100 rows of the LDS classes, above 64 KB among them"""
    edges = [k for k, s in enumerate(R.BLOCK_EDGES) if 64 < min(s) + 1 <= 128]
    lds = [2 * i + j for i, (rows, _) in enumerate(R.LDS_SHAPES) if rows == 100 for j in (0, 1)]
    small = [2 * i + j for i, rows in enumerate(R.SMALL_LDS_ROWS) if rows == 100 for j in (0, 1)]
    assert len(edges) == 4 and len(lds) == 4 and len(small) == 2
    if which == "small":
        return capi.StitchBatch.concat([R.batch_of("edges_dags").subset(edges[:2]), R.batch_of("small_lds").subset(small)])
    return capi.StitchBatch.concat([R.batch_of("edges_dags").subset(edges), R.batch_of("edges_dense_dags").subset(edges), R.batch_of("lds_classes").subset(lds)])


def _digest(res):
    h = hashlib.sha256()
    for f in ("aln_off", "pairs", "score", "route", "num_pw"):
        h.update(np.ascontiguousarray(getattr(res, f)).tobytes())
    return h.hexdigest()


_BLOCK128_CHILD = """
import sys, json
sys.path.insert(0, ROOT_DIR)
import numpy as np
from centrolign_amd import capi
from tests import test_gpu_sys_kernel as T
ctx = capi.Context(0)
out = []
for which in ("small", "large"):
    b = T._block128_batch(which)
    for npw in (1, 2, 3):
        plan = ctx.plan(b, force_num_pw=np.full(b.n_problems, npw, np.uint8))
        launches = [(li["kernel"], li["n_problems"], li["lds_bytes"]) for li in plan.launches() if li["n_problems"]]
        plan.execute(); plan.sync()
        out.append(dict(which=which, npw=npw, launches=launches, digest=T._digest(plan.collect())))
        plan.destroy()
ctx.close()
print(json.dumps(out))
"""


def test_the_128_thread_instantiations(gpu_ctx, monkeypatch):
    """CL_SYS_BLOCK128=1 gives pairs of 65 to 128 rows two waves instead of four.  One fresh child process with a time limit of its own makes the three plans, which
    must consist of popoa_sys_kernel<n, 128> with the LDS the rule predicts, and its bytes must be the ones this process gets from the 256-thread instantiations —
    which are the oracle's"""
    env = dict(os.environ, CL_SYS_BLOCK128="1", CL_NO_LANE="1")
    for name in HOOK_NAMES:
        if name != "CL_NO_LANE":
            env.pop(name, None)
    r = subprocess.run([sys.executable, "-c", "ROOT_DIR = %r\n" % ROOT + _BLOCK128_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads(r.stdout.strip().splitlines()[-1])
    assert [(x["which"], x["npw"]) for x in child] == [(w, n) for w in ("small", "large") for n in (1, 2, 3)]
    for x in child:
        npw, b = x["npw"], _block128_batch(x["which"])
        f = np.full(b.n_problems, npw, np.uint8)
        want128, taken = R.predicted_launches(b, f, block128=True)
        got128 = sorted(tuple(li) for li in x["launches"] if li[0].startswith(R.SYS))
        assert len(taken) >= b.n_problems - 2 and got128 == want128 == [("popoa_sys_kernel<%d, 128>" % npw, len(taken), want128[0][2])], (x, want128)
        plan, launches = _plan(gpu_ctx, monkeypatch, "block128", b, f)
        assert [li[0] for li in launches] == ["popoa_sys_kernel<%d, 256>" % npw] and launches[0][1:] == want128[0][1:], (launches, want128)
        plan.execute(); plan.sync()
        got = plan.collect()
        plan.destroy()
        assert got.same_as(po.oracle_stitch_batch(b, force_num_pw=f)) is None
        assert _digest(got) == x["digest"], "NumPW %d: popoa_sys_kernel<%d, 128> and <%d, 256> give different bytes" % (npw, npw, npw)
        assert (want128[0][2] > R.LDS_SPLIT) == (x["which"] == "large")
        _seen[("block128 " + x["which"], "auto", npw)] = want128


# ---- a mixed batch, resident ------------------------------------------------------------------------------------------------------------------------------------
def test_a_resident_plan_gives_the_same_bytes_every_time(gpu_ctx, monkeypatch):
    """every group's small pairs in one plan, NumPW 1, 2, 3 in turn; the LDS classes of a workgroup size share a launch (host-only: tests/test_sys_rule.py)"""
    small = lambda group: [k for k in range(R.batch_of(group).n_problems) if max(int(x[k]) for x in R.batch_of(group).sizes()) <= 450]
    b = capi.StitchBatch.concat([R.batch_of(g).subset(small(g)) for g in ("lds_classes", "edges_dags", "saved_columns", "cells", "ring_depth", "random_dags")])
    f = (np.arange(b.n_problems) % 3 + 1).astype(np.uint8)
    want = po.oracle_stitch_batch(b, force_num_pw=f)
    plan, launches = _plan(gpu_ctx, monkeypatch, "mixed", b, f)
    assert len(launches) >= 6 and sum(li[1] for li in launches) >= 100, launches
    first = None
    for _ in range(3):
        plan.execute(); plan.sync()
        got = plan.collect()
        assert got.same_as(want) is None
        first = first or got
        assert _same_bytes(got, first)
    plan.destroy()


# ---- what ran -------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_ring_depth_and_saved_column_count(gpu_ctx, monkeypatch):
    """over the plans of test_against_the_oracle and of the child of the 128-thread test (planned again here where those did not run before this one, the 128-thread
    launches then taken from the rule): all twelve popoa_sys_kernel<NPW, BLOCK>, each with at most 64 KB and with more of dynamic LDS; every log2 H from 2 to 12 at
    NumPW 1 and to 10 at NumPW 2 and 3 (11 needs a near distance above 1 022 beside 128 KB of ring: tests/test_sys_rule.py); 0, 1, 2, 3 and 32 saved columns and
    column 0 among them.  Nothing the rule can reach is missing.  Prints the sets (pytest -s)"""
    classes, logs, saved, col0 = {}, {1: set(), 2: set(), 3: set()}, set(), False
    for group, order in R.runs():
        b = R.batch_of(group)
        for npw in (1, 2, 3):
            f = np.full(b.n_problems, npw, np.uint8)
            if (group, order, npw) not in _seen:
                plan, launches = _plan(gpu_ctx, monkeypatch, group, b, f, order=order)
                plan.destroy()
                _seen[(group, order, npw)] = launches
            for k in R.predicted_launches(b, f, order, force_general=group in R.FORCE_GENERAL)[1]:
                c = R.sys_rule(b, k, npw, order)[0]
                logs[npw].add(c["log2_depth"])
                saved.add(len(c["saved"]))
                col0 |= bool(c["saved"]) and c["saved"][0] == 0
    for which in ("small", "large"):
        b = _block128_batch(which)
        for npw in (1, 2, 3):
            _seen.setdefault(("block128 " + which, "auto", npw), R.predicted_launches(b, np.full(b.n_problems, npw, np.uint8), block128=True)[0])
    for (group, order, npw), launches in _seen.items():
        for kernel, count, lds in launches:
            classes.setdefault((kernel, lds > R.LDS_SPLIT), []).append((group, lds))
    print("\npopoa_sys_kernel launches (instantiation, above 64 KB of dynamic LDS): largest LDS, groups")
    for key in sorted(classes):
        print("  %-28s %-5s %6d bytes   %s" % (key + (max(x[1] for x in classes[key]), " ".join(sorted({x[0] for x in classes[key]})))))
    print("log2 H by NumPW: %r; saved columns per pair: %r" % ({k: sorted(v) for k, v in logs.items()}, sorted(saved)))
    for npw in (1, 2, 3):
        for block in (64, 128, 256, 1024):
            for big in (False, True):
                # a launch's LDS is that of its hungriest member: the class of at most 64 KB shows where a plan holds no larger pair of that workgroup size
                assert ("popoa_sys_kernel<%d, %d>" % (npw, block), big) in classes, (npw, block, big)
    assert logs[1] == set(range(2, 13)) and logs[2] == logs[3] == set(range(2, 11)), logs
    assert {0, 1, 2, 3, 32} <= saved and max(saved) == 32 and col0, saved
