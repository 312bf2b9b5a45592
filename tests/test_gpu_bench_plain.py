"""A plain `bench.py` run (no --full) at a dry-run length: the line carries the headline and nothing that needs a measurement of its own, and --dump-outputs
still writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("timed_blocks", "msa_wall_s_second_run", "msa", "with_a_join_per_pass", "launches", "roofline", "roofline_pass", "in_situ",
             "cpu_baseline", "cpu_reference_wall", "chaining_c2", "pairwise_c2", "big_dag_pair")


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_alone(tmp_path):
    dump = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--length", "30000", "--dump-outputs", dump]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "DP cells/s" and out["higher_is_better"] is True and out["dtype"] == "int32" and out["metric"].startswith("stitcher PO-POA DP cells/s")
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - out["config"]["dp_cells"] / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert out["config"]["workload"].startswith("DRY RUN at 30000 bp")
    assert [k for k in FULL_ONLY if k in out] == []
    assert "other_plan_layout" not in out["config"] and out["config"]["gfa_sha256"] is None
    for name in ("stitch_score", "stitch_aln_len", "stitch_route", "stitch_num_pw", "stitch_pairs"):
        assert np.load(os.path.join(dump, name + ".npy")).size > 0
