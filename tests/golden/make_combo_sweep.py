"""Expected values of the chaining DP across the number of chain combinations -> tests/golden/chain_combo_sweep.npz.

For every case of tests/helpers.py:combo_cases() the file holds a sha256 of the regenerated inputs (a drifting generator is noticed) and the number of chain
combinations counted from them in Python.  For the cases whose oracle run is too slow for a test (helpers.combo_oracle_is_live: more than about 2 s) it also
holds the oracle's affine DP values as uint32 bit patterns and its chain, under global anchoring, and under local anchoring too for the small and tiny sizes.
Where the compiled reference is built (oracle/_ref), the chain of its sparse_affine_chain_dp on the same input is recorded beside the oracle's, and the two
are asserted equal before anything is written — on the cases with fewer than 256 paths on either side: with 256 and more the compiled reference did not finish
within two minutes on an input the oracle takes 0.9 s for (1 x 257 paths, 300 pairs), so those cases carry the oracle's values alone.  Inputs are not stored:
they are rebuilt from their seeds.

usage: python tests/golden/make_combo_sweep.py [jobs [case ...]]      (from the repository root; with case names: only those, merged into the file)
Measured: 11.5 min with 7 jobs on 8 cores (the 32 x 33 multi-block case alone takes 10 min: oracle and compiled reference), about 10 GB for that job."""
import os
import sys
import time
from multiprocessing import get_context

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from oracle import pyoracle as po  # noqa: E402
from tests import helpers as H  # noqa: E402

OUT = os.path.join(H.GOLDEN, "chain_combo_sweep.npz")


def anchorings(case):
    return (True,) if case.size == "multi" else (True, False)


def one_case(name):
    case = H.combo_case(name)
    t0 = time.time()
    g1, g2, ms, scale = H.combo_input(case)
    out = {name + "/digest": np.array(H.combo_input_digest(g1, g2, ms, scale)), name + "/combos": np.array(H.count_combinations(g1, g2, ms), np.int64),
           name + "/pairs": np.array(ms.n_pairs(), np.int64)}
    assert int(out[name + "/combos"]) == case.combos, (name, int(out[name + "/combos"]))
    if not H.combo_oracle_is_live(case):
        for glob in anchorings(case):
            pre = "%s/%s/" % (name, "global" if glob else "local")
            chain, dp = po.oracle_chain("affine", g1, g2, ms, scale=scale, want_dp=True, global_anchoring=glob)
            out[pre + "dp"] = dp[:ms.n_pairs()].view(np.uint32).copy()
            out[pre + "chain"] = chain.astype(np.uint32)
            if po.have_ref() and H.combo_ref_can_run(case):
                ref, _ = po.ref_chain("affine", g1, g2, ms, scale=scale, global_anchoring=glob)
                assert np.array_equal(ref, chain), "%s: the compiled reference's chain differs from the oracle's" % pre
                out[pre + "ref_chain"] = ref.astype(np.uint32)
    print("%-16s %5d pairs %6d combinations  %.1f s" % (name, ms.n_pairs(), case.combos, time.time() - t0), flush=True)
    return out


def main():
    jobs = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    t0 = time.time()
    only = sys.argv[2:]
    cases = sorted((c for c in H.combo_cases() if not only or c.name in only), key=lambda c: -c.combos * c.pairs)      # the longest first
    with get_context("spawn").Pool(jobs, maxtasksperchild=1) as pool:
        parts = pool.map(one_case, [c.name for c in cases], chunksize=1)
    d = {}
    if only:
        with np.load(OUT) as z:
            d = {k: z[k] for k in z.files}
    for p in parts:
        d.update(p)
    np.savez_compressed(OUT, **d)
    print("%s: %d bytes, %.0f s, compiled reference %s" % (OUT, os.path.getsize(OUT), time.time() - t0, "recorded" if po.have_ref() else "absent"))


if __name__ == "__main__":
    main()
