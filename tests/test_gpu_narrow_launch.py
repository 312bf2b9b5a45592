"""In plans of 2 048 subproblems and more, the stitch pass's launches of few workgroups (popoa_lane_kernel<1 / 3 / 4>, small popoa_sys_kernel<NPW, 64 / 256> launches)
run as ONE launch, popoa_narrow_kernel, as long as all its workgroups are resident at once.  Every workgroup runs the body of its own launch on the same pair, so the
results are the same bytes.  CL_STITCH_NARROW=0 keeps the separate launches; the switch is read once per process, so every case runs in two child processes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_CASE = """
import hashlib, json, sys
sys.path.insert(0, ROOT_DIR)
import numpy as np
from centrolign_amd import capi, synth
from oracle import pyoracle as po

def digest(res):
    h = hashlib.sha256()
    for a in (res.aln_off, res.pairs, res.score, res.route, res.num_pw):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()

def kernels(plan):
    return sorted(set(li["kernel"] for li in plan.launches() if li["n_problems"]))

# near-chain pairs of <= 64 rows (one wave) and 65-192 rows (a round of three waves, four with CL_LANE_WAVES=4), both orientations; p_del 0.08 gives
# row predecessors up to four ranks back (the second cell shape)
near = []
for k, (p_del, seed) in enumerate(((0.03, 40), (0.08, 41))):
    near.append(synth.near_chain_batch([(40, 900), (900, 50), (64, 700), (130, 800), (800, 150), (190, 600), (100, 1200), (20, 640)], seed=seed, p_del=p_del,
                                       n_long=(0, 1)))
# DAG pairs for the systolic kernel: <= 64 rows (64 threads), 65-256 rows (256 threads), in two LDS classes
dags = [synth.random_dag_batch(300, seed=42, max_n=60), synth.sized_dag_batch([(120, 300), (200, 1400), (90, 150), (250, 900)], seed=43),
        synth.sized_dag_batch([(40, 60), (60, 1800)], seed=44)]
# a chain pair long enough to span several workgroups (CL_SPAN_DEBUG_FAIL=1 makes it report status 9, and collect runs it again)
span = synth.linear_batch([(2600, 2500)], seed=45)
head = capi.StitchBatch.concat(near + dags + [span])
rng = np.random.default_rng(46)
fill = synth.linear_batch([(int(rng.integers(4, 60)), int(rng.integers(4, 200))) for _ in range(2100 - head.n_problems)], seed=47)
big = capi.StitchBatch.concat([head, fill])
npw = np.array([1 + i % 3 for i in range(big.n_problems)], np.uint8)   # every NumPW on every kind

ctx = capi.Context(0)
out = {}
plan = ctx.plan(big, force_num_pw=npw)
out["kernels"] = kernels(plan)
out["narrow_members"] = [li["n_problems"] for li in plan.launches() if li["kernel"] == "popoa_narrow_kernel"]
plan.execute(); plan.sync()
first = plan.collect()
out["big"] = digest(first)
out["oracle"] = first.same_as(po.oracle_stitch_batch(big, force_num_pw=npw)) is None
out["passes_equal"] = True
for _ in range(3):
    for _ in range(5):
        plan.execute()
    plan.sync()
    out["passes_equal"] = out["passes_equal"] and digest(plan.collect()) == out["big"]
plan.execute_profiled(); plan.sync()
out["profiled_equal"] = digest(plan.collect()) == out["big"]
plan.destroy()
# below 2 048 subproblems nothing is merged
small = capi.StitchBatch.concat(near + dags)
plan = ctx.plan(small)
out["small_kernels"] = kernels(plan)
plan.execute(); plan.sync()
out["small"] = digest(plan.collect())
plan.destroy()
ctx.close()
print(json.dumps(out))
"""


def _run(narrow, extra_env):
    env = dict(os.environ, CL_STITCH_NARROW="1" if narrow else "0", CL_LANE_MIN_SWEEP="0", CL_STITCH_DEBUG_CLEAR="1", CL_SPAN_DEBUG_FAIL="1", **extra_env)
    r = subprocess.run([sys.executable, "-c", "ROOT_DIR = %r\n" % ROOT + _CASE], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("lane_waves", ["3", "4"])
def test_narrow_launch_matches_the_separate_launches(lane_waves):
    new, old = _run(True, dict(CL_LANE_WAVES=lane_waves)), _run(False, dict(CL_LANE_WAVES=lane_waves))
    assert "popoa_narrow_kernel" in new["kernels"], new["kernels"]
    assert "popoa_narrow_kernel" not in old["kernels"], old["kernels"]
    assert {"popoa_lane_kernel<1>", "popoa_lane_kernel<%s>" % lane_waves} <= set(old["kernels"]), old["kernels"]
    assert len(new["kernels"]) < len(old["kernels"]), (new["kernels"], old["kernels"])
    for run in (new, old):
        assert run["oracle"] and run["passes_equal"] and run["profiled_equal"], run
        assert "popoa_narrow_kernel" not in run["small_kernels"], run["small_kernels"]
    assert new["big"] == old["big"] and new["small"] == old["small"]
