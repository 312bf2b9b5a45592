"""A stitch plan of more than two launches that is executed again deals its launches over the streams anew: in front of its second pass by the durations measured alone,
in front of its third by the launches' own clocks inside the pass before (cl_stitch_plan_execute).  A re-deal reorders the launch groups and nothing else: every pass
computes what the oracle computes, and every group keeps its list.  The switches involved are read once per process, so the case runs in a child process
(as in tests/test_gpu_persistent_pass.py): one launch per kernel shape (CL_STITCH_PERSISTENT=0, CL_STITCH_NARROW=0) and outputs zeroed in front of every pass
(CL_STITCH_DEBUG_CLEAR=1), so that a launch a pass lost shows up as zero lengths and scores, not as the pass before."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

N_PASSES = 5

# the smallest batch with a launch per kind: chain pairs of at most 16 rows (four per wave) and of 65-256 rows (four waves), branching pairs of at most 64 and of 129-256
# rows (two workgroup sizes of the DAG kernels), a near-chain pair
_CHILD = """
import json, sys
sys.path.insert(0, ROOT_DIR)
import numpy as np
from centrolign_amd import capi, synth
from oracle import pyoracle as po

batch = capi.StitchBatch.concat([synth.linear_batch([(12, 40), (30, 16)], seed=1), synth.linear_batch([(200, 230), (120, 100)], seed=2),
                                 synth.sized_dag_batch([(50, 60), (40, 30)], seed=3), synth.sized_dag_batch([(200, 180), (150, 240)], seed=4),
                                 synth.near_chain_batch([(300, 320)], seed=5)])
want = po.oracle_stitch_batch(batch)
ctx = capi.Context(0)
plan = ctx.plan(batch)
out = dict(launch_count=len(plan.launches()), diffs=[], lists=[])
for _ in range(N_PASSES):
    plan.execute()
    plan.sync()
    out["diffs"].append(plan.collect().same_as(want))
    out["lists"].append(sorted((li["kernel"], li["n_problems"], li["dp_cells"]) for li in plan.launches()))
plan.destroy()
ctx.close()
print(json.dumps(out))
"""


def test_redealt_passes_match_the_oracle_and_keep_their_lists():
    env = dict(os.environ, CL_STITCH_PERSISTENT="0", CL_STITCH_NARROW="0", CL_STITCH_DEBUG_CLEAR="1")
    code = "ROOT_DIR = %r\nN_PASSES = %d\n" % (ROOT, N_PASSES) + _CHILD
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["launch_count"] > 2, "the batch must yield more than two launches, or no pass is re-dealt: %d" % out["launch_count"]
    assert len(out["diffs"]) == N_PASSES
    for i, diff in enumerate(out["diffs"]):
        assert diff is None, "pass %d differs from the oracle: %s" % (i + 1, diff)
    for i, lst in enumerate(out["lists"]):
        assert len(lst) == out["launch_count"]
        assert lst == out["lists"][0], "pass %d: the launch groups are not those of the first pass" % (i + 1)
