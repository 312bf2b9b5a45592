"""GPU suite: a chaining DP gives back every device block it took.  The DP's buffers and events have one owner that lets go of them at scope exit, whichever
way the DP ends; here the device bytes a context holds (cl_context_memory, live bytes) are read before and after a DP on its paths through that owner: the
packed block of a small DP, the separate arrays of a larger one, the factored queries and far-pass structures of a multi-block one, an input that is refused before the device is touched, and the walk kernel's stall (the test
hook CL_CHAIN_DEBUG_STALL=1: the attempt on the walk kernels ends early with kWalkStalled, the DP is run again on the per-block kernels)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from centrolign_amd import capi
from tests import helpers as H
from tests.test_extraction import load_stitch_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# the smallest inputs of the combination sweep on each side of the 2 MB up to which a DP's arrays travel in one block: 300 pairs in one combination
# (about 20 KB) and in 256 combinations (13 KB of queries and results each: 3.4 MB); and the smallest input whose queries go up as factors, in a few blocks for all
# combinations, and whose five macro-blocks run the far pass with its arena, orders and sealing schedule
@pytest.mark.parametrize("name, arrays, queries, far", [("1x1_small", "packed", "dense", "off"), ("16x16_small", "separate", "dense", "off"),
                                                        ("16x16_multi", "separate", "factored", "on")])
def test_a_dp_returns_the_device_memory_it_took(gpu_ctx, monkeypatch, capfd, name, arrays, queries, far):
    g1, g2, ms, scale = H.combo_input(H.combo_case(name))
    monkeypatch.setenv("CL_CHAIN_TIMING", "1")   # (read at every call)
    before = gpu_ctx.memory_stats()["live_bytes"]
    capfd.readouterr()
    got = gpu_ctx.chain_sparse_affine(g1, g2, ms, scale=scale, params=capi.default_chain_params(global_anchoring=True))
    err = capfd.readouterr().err
    after = gpu_ctx.memory_stats()["live_bytes"]
    held = float(re.findall(r"device memory held by the context: ([\d.]+) MB", err)[-1])
    with capfd.disabled():
        print("%s: live bytes before %d, after %d; %.1f MB held during the DP" % (name, before, after, held))
    assert re.findall(r"arrays (\w+)", err)[-1] == arrays
    assert re.findall(r"\((\w+) queries, far pass (\w+):", err)[-1] == (queries, far)
    assert len(got["chain"]) > 0
    assert after == before


def test_a_refused_dp_holds_no_device_memory(gpu_ctx):
    name = sorted(f for f in os.listdir(H.GOLDEN) if f.startswith("chain4_"))[0]
    z = np.load(os.path.join(H.GOLDEN, name))
    _, graphs, _ = load_stitch_case(name.replace("chain4_", "stitch4_"))
    bad = capi.MatchSets(**{k: z["a.ms." + k].copy() for k in capi.MatchSets._DT})
    bad.nodes1[-1] = len(graphs[0].label) + 7
    before = gpu_ctx.memory_stats()["live_bytes"]
    with pytest.raises(capi.ClError) as e:
        gpu_ctx.chain_sparse_affine(graphs[0], graphs[1], bad)
    assert "node id outside its graph" in str(e.value)
    after = gpu_ctx.memory_stats()["live_bytes"]
    assert after == before


def test_a_stalled_walk_returns_its_device_memory():
    """CL_CHAIN_DEBUG_STALL is read once: a child process, as in test_gpu_chain.py::test_walk_stall_falls_back_to_the_per_block_kernels"""
    code = (
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from centrolign_amd import capi\n"
        "from tests import helpers as H\n"
        "from tests.test_extraction import load_stitch_case\n"
        "name = sorted(f for f in os.listdir(H.GOLDEN) if f.startswith('chain4_'))[-1]\n"
        "z = np.load(os.path.join(H.GOLDEN, name))\n"
        "_, graphs, _ = load_stitch_case(name.replace('chain4_', 'stitch4_'))\n"
        "ctx = capi.Context(0)\n"
        "ms = capi.MatchSets(**{k: z['a.ms.%%s' %% k] for k in capi.MatchSets._DT})\n"
        "before = ctx.memory_stats()['live_bytes']\n"
        "got = ctx.chain_sparse_affine(graphs[0], graphs[1], ms, scale=float(z['a.scale'][0]), params=capi.default_chain_params(global_anchoring=True))\n"
        "assert np.array_equal(got['chain'], z['a.chain_affine_global'])\n"
        "print('LIVE %%d %%d' %% (before, ctx.memory_stats()['live_bytes']))\n" % ROOT)
    env = dict(os.environ, CL_CHAIN_DEBUG_STALL="1", CL_CHAIN_TIMING="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "walk kernel stalled: repeating the DP on the per-block kernels" in r.stderr and "path: per-block" in r.stderr
    before, after = [int(x) for x in re.search(r"LIVE (\d+) (\d+)", r.stdout).groups()]
    assert after == before
