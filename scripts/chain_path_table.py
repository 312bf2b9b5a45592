"""Which way the chaining DP goes, input by input and switch set by switch set: every input of the combination sweep (tests/helpers.py: combo_cases) under the default
switches and under the switch sets of tests/test_gpu_far_modes.py, each in a child process (tests/far_ab_child.py: the switches are read once per process) with a time
limit of its own; the first child that fails or runs out of time ends the run.  One row per run: the path line, the memory line's queries / far pass / walk fields, how the
traceback got its rows, and the digests of the DP values and of the chain.  Two builds of the library decide alike exactly when their tables are the same bytes
(profiles/chain_path_table.txt is the table of the current sources).

usage: python scripts/chain_path_table.py [--cases NAME,...] [--variant-cases NAME,...] [--kinds affine,sparse] [--timeout S] > table.txt
  --cases          inputs run under the default switches (default: all)
  --variant-cases  inputs run under every switch set as well (default: all; every set on every input is some 2 500 processes)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import far_ab_child, helpers as H  # noqa: E402
from tests.test_gpu_far_modes import VARIANTS  # noqa: E402

SWITCHES = sorted({k for _, env in VARIANTS for k in env} | {"CL_CHAIN_GROUP_PATH", "CL_CHAIN_DEBUG_STALL"})


def run(path, kind, env_extra, timeout):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra, CL_CHAIN_TIMING="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "far_ab_child.py"), path, kind], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("exit status %d\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:]))
    path_line = re.findall(r"\[chain_dp_batch\]\s+(path: .*)\n", r.stderr)[-1]
    queries, far, walk = re.findall(r"device memory held by the context: [\d.]+ MB \((\w+) queries, far pass (\w+): .*, walk (\w+)\)", r.stderr)[-1]
    rows = re.findall(r"\[chain_dp_batch\]\s+traceback rows ([\w ]+)\n", r.stderr)[-1]
    dp, chain = re.search(r"RESULT pairs=\d+ anchors=\d+ dp=(\w+) chain=(\w+)", r.stdout).groups()
    return "%s | queries %s, far pass %s, walk %s | rows %s | dp %s chain %s" % (path_line, queries, far, walk, rows, dp[:16], chain[:16])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="")
    ap.add_argument("--variant-cases", default=None)
    ap.add_argument("--kinds", default="affine,sparse")
    ap.add_argument("--timeout", type=float, default=120.0)
    a = ap.parse_args()
    cases = [c for c in H.combo_cases() if not a.cases or c.name in a.cases.split(",")]
    with_variants = None if a.variant_cases is None else set(a.variant_cases.split(","))
    with tempfile.TemporaryDirectory() as tmp:
        for case in cases:
            path = os.path.join(tmp, case.name + ".npz")
            far_ab_child.save_input(path, *H.combo_input(case))
            for name, env in VARIANTS:
                if env and with_variants is not None and case.name not in with_variants:
                    continue
                for kind in a.kinds.split(","):
                    try:
                        row = run(path, kind, env, a.timeout)
                    except (RuntimeError, subprocess.TimeoutExpired) as e:
                        print("%-16s %-28s %-6s FAILED: %s" % (case.name, name, kind, e), flush=True)
                        sys.exit(1)
                    print("%-16s %-28s %-6s %s" % (case.name, name, kind, row), flush=True)


if __name__ == "__main__":
    main()
