"""Child process of tests/test_gpu_pair_sweep.py: the chaining DP's switches are read once per process, so every setting runs in a process of its own — but on
a whole LIST of saved inputs (tests/far_ab_child.py:save_input), the affine and the gap-free DP on each, global anchoring.  A "CASE <name> <algo>" line on stderr
stands in front of each run's CL_CHAIN_TIMING log, and each run prints one line

    RESULT case=<name> algo=<algo> pairs=<n> anchors=<n> dp=<sha256> chain=<sha256> changed=<n>

on stdout; `changed` counts the DP values that differ from the ones the input carries as "want.<algo>" (uint32 bit patterns), -1 where it carries none.

usage: python tests/pair_sweep_child.py NAME=INPUT.npz [NAME=INPUT.npz ...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from centrolign_amd import capi  # noqa: E402
from tests import far_ab_child  # noqa: E402

ALGOS = ("affine", "sparse")


def main():
    ctx = capi.Context(0)
    for arg in sys.argv[1:]:
        name, path = arg.split("=", 1)
        g1, g2, ms, scale = far_ab_child.load_input(path)
        z = np.load(path)
        for algo in ALGOS:
            print("CASE %s %s" % (name, algo), file=sys.stderr, flush=True)
            got = ctx.chain_sparse_affine(g1, g2, ms, scale=scale, want_dp=True, sparse=algo == "sparse", params=capi.default_chain_params(global_anchoring=True))
            dp = got["dp"] if got["dp"] is not None else np.zeros(0, np.float32)
            changed = -1
            if "want." + algo in z.files and len(z["want." + algo]) == len(dp):
                changed = int(np.count_nonzero(dp.view(np.uint32) != z["want." + algo]))
            print("RESULT case=%s algo=%s pairs=%d anchors=%d dp=%s chain=%s changed=%d" % ((name, algo, got["n_pairs"], len(got["chain"])) + far_ab_child.digests(dp, got["chain"]) + (changed,)),
                  flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
