"""The one-wave chain kinds of a stitch pass (popoa_linear_kernel<1>, the quads, the duos) run as ONE persistent launch that pulls its tasks from a device-side list
(popoa_chain_persistent_kernel).  CL_STITCH_PERSISTENT=0 keeps one launch per kind.  The switch is read once per process, so every case runs in two child processes,
one per setting, and the two must compute the same bytes (and, where the batch is small enough, what the oracle computes)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

_PRELUDE = """
import hashlib, json, sys, threading
sys.path.insert(0, ROOT_DIR)
import numpy as np
from centrolign_amd import capi, synth

def digest(res):
    h = hashlib.sha256()
    for a in (res.aln_off, res.pairs, res.score, res.route, res.num_pw):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()

def small_chains(n, seed):
    rng = np.random.default_rng(seed)
    sizes = []
    for i in range(n):
        r = int(rng.integers(1, 65))                      # quads (<= 16 rows), duos (17-32), single pairs (33-64)
        c = int(rng.integers(r, 3 * r + 40))
        sizes.append((r, c) if i % 2 else (c, r))
    return synth.linear_batch(sizes, seed=seed)

out = {}
"""

CASES = {
    # every kernel kind of the stitch path in one batch: DAG pairs (systolic / general / ring), near-chain pairs (lane), chain pairs of every size (one-wave kinds,
    # linear<W>), beside a batch whose large branching pairs take the strip kernel
    "every_kind": """
ctx = capi.Context(0)
mixed = capi.StitchBatch.concat([synth.random_dag_batch(200, seed=3, max_n=120), synth.near_chain_batch([(300, 320), (60, 70), (900, 880), (40, 45)], seed=4),
                                 small_chains(600, 5), synth.linear_batch([(200, 210), (700, 650), (1500, 1400), (3000, 2900)], seed=6)])
plan = ctx.plan(mixed)
out["kernels"] = sorted(set(li["kernel"].split("<")[0] for li in plan.launches()))
plan.execute(); plan.sync()
out["mixed"] = digest(plan.collect())
plan.destroy()
strips = synth.sized_dag_batch([(900, 700), (1300, 800), (600, 2000), (2000, 600), (700, 700)], seed=33, extra_edge_p=0.05, skip_max=3)
plan = ctx.plan(strips)
out["strip_kernels"] = sorted(set(li["kernel"].split("<")[0] for li in plan.launches()))
plan.execute(); plan.sync()
out["strips"] = digest(plan.collect())
plan.destroy()
ctx.close()
""",
    # more tasks than the persistent grid has workgroups (quads of 16 rows and ~600 columns: one quad per task), then many back-to-back passes of one plan
    # (the queue words are re-armed by the launch itself, not by a memset).  Run with CL_STITCH_DEBUG_CLEAR=1: every pass starts from zeroed outputs, so a pass
    # whose launch found its queue words not re-armed (and skipped every task) would leave zero lengths and scores behind, not the previous pass's results
    "many_tasks_and_passes": """
ctx = capi.Context(0)
rng = np.random.default_rng(8)
sizes = [(int(rng.integers(8, 17)), int(rng.integers(560, 640))) for _ in range(16000)] + [(int(rng.integers(33, 65)), int(rng.integers(100, 400))) for _ in range(3000)]
b = synth.linear_batch(sizes, seed=9)
plan = ctx.plan(b)
out["kernels"] = sorted(set(li["kernel"].split("<")[0] for li in plan.launches()))
plan.execute(); plan.sync()
first = digest(plan.collect())
out["passes_equal"] = True
for rnd in range(4):
    for _ in range(10):
        plan.execute()
    plan.sync()
    out["passes_equal"] = out["passes_equal"] and digest(plan.collect()) == first
plan.execute_profiled(); plan.sync()
out["profiled_equal"] = digest(plan.collect()) == first
out["many"] = first
plan.destroy()
ctx.close()
""",
    # a batch with one subproblem and a batch of quads only keep their kind's own launch (one kind: nothing to merge, by design); a batch of single pairs and
    # duos but no quads takes the persistent launch with one kind absent from its task list
    "small_batches": """
ctx = capi.Context(0)
from oracle import pyoracle as po
for name, b in (("one", synth.linear_batch([(40, 57)], seed=1)), ("quads_only", synth.linear_batch([(5, 30), (12, 9), (16, 40), (3, 3), (9, 70)], seed=2)),
                ("no_quads", synth.linear_batch([(20, 31), (48, 60), (64, 64), (25, 90), (33, 47)], seed=3))):
    plan = ctx.plan(b)
    out[name + "_kernels"] = sorted(set(li["kernel"].split("<")[0] for li in plan.launches()))
    plan.destroy()
    got = ctx.stitch_batch_align(b)
    out[name] = digest(got)
    out[name + "_oracle"] = got.same_as(po.oracle_stitch_batch(b)) is None
ctx.close()
""",
    # two plans on two contexts executing at once, as the MSA's worker contexts do (CL_STITCH_DEBUG_CLEAR=1: every pass recomputes what is compared)
    "two_contexts": """
res = {}
def work(k):
    ctx = capi.Context(0)
    plan = ctx.plan(small_chains(3000, 20 + k))
    for _ in range(15):
        plan.execute()
    plan.sync()
    res[k] = digest(plan.collect())
    plan.destroy()
    ctx.close()
ts = [threading.Thread(target=work, args=(k,)) for k in range(2)]
for t in ts: t.start()
for t in ts: t.join()
out["ctx0"], out["ctx1"] = res[0], res[1]
""",
}


def _run(case, persistent, extra_env=None):
    env = dict(os.environ, CL_STITCH_PERSISTENT="1" if persistent else "0", **(extra_env or {}))
    code = "ROOT_DIR = %r\n" % ROOT + _PRELUDE + CASES[case] + "\nprint(json.dumps(out))\n"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _compare(case, keys, extra_env=None):
    new, old = _run(case, True, extra_env), _run(case, False, extra_env)
    for k in keys:
        assert new[k] == old[k], (case, k)
    return new, old


def test_every_kernel_kind_matches_the_per_kind_launches():
    new, old = _compare("every_kind", ("mixed", "strips"))
    assert "popoa_chain_persistent_kernel" in new["kernels"], new["kernels"]
    assert "popoa_chain_persistent_kernel" not in old["kernels"], old["kernels"]
    for k in ("popoa_linear_kernel", "popoa_linear_quad_kernel", "popoa_linear_duo_kernel"):
        assert k in old["kernels"], (k, old["kernels"])


def test_strip_and_spanning_pairs_keep_their_own_launches():
    # (CL_NO_LANE=1 as in test_gpu_parity: the large branching pairs take the strips; the chain pair of 3 000 x 2 900 spans several workgroups)
    new, old = _compare("every_kind", ("mixed", "strips"), dict(CL_NO_LANE="1"))
    for run in (new, old):
        assert "popoa_linear_span_kernel" in run["kernels"], run["kernels"]
        assert "popoa_strip_kernel" in run["strip_kernels"], run["strip_kernels"]
    assert "popoa_chain_persistent_kernel" in new["kernels"]


def test_more_tasks_than_workgroups_and_many_passes():
    new, old = _compare("many_tasks_and_passes", ("many",), dict(CL_STITCH_DEBUG_CLEAR="1"))
    assert "popoa_chain_persistent_kernel" in new["kernels"]
    assert new["passes_equal"] and new["profiled_equal"] and old["passes_equal"]


def test_single_subproblem_and_kinds_without_tasks():
    new, old = _compare("small_batches", ("one", "quads_only", "no_quads"))
    for name in ("one", "quads_only", "no_quads"):
        assert new[name + "_oracle"], (name, new)
        assert "popoa_chain_persistent_kernel" not in old[name + "_kernels"], (name, old[name + "_kernels"])
    assert new["one_kernels"] == ["popoa_linear_kernel"] and new["quads_only_kernels"] == ["popoa_linear_quad_kernel"], new
    assert new["no_quads_kernels"] == ["popoa_chain_persistent_kernel"], new["no_quads_kernels"]


def test_two_contexts_at_once():
    _compare("two_contexts", ("ctx0", "ctx1"), dict(CL_STITCH_DEBUG_CLEAR="1"))
