"""The inputs and expected values of the chaining DP's sweep over the number of chain combinations (tests/helpers.py:combo_cases(),
tests/golden/chain_combo_sweep.npz, written by tests/golden/make_combo_sweep.py): the generator has not drifted, every case has the number of combinations it
states, the oracle reproduces the golden, and so does the compiled reference where it is built.  The device side is tests/test_gpu_combo_sweep.py."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H

CASES = H.combo_cases()
_Z = {}
# the stored cases the oracle can still be run on here (about 2 s each: one macro-block, 512 and 513 combinations); the rest of the file took minutes to compute
RERUN = ["16x32_small", "19x27_small"]


def golden():
    if "z" not in _Z:
        _Z["z"] = np.load(os.path.join(H.GOLDEN, "chain_combo_sweep.npz"))
    return _Z["z"]


def test_the_cases_stand_on_both_sides_of_every_threshold():
    counts = sorted({c.combos for c in CASES})
    assert counts == [1, 2, 4, 8, 9, 16, 17, 18, 256, 257, 512, 513, 768, 770, 1056, 4096, 4160, 65535, 65536, 65792]
    for n in counts:
        sizes = sorted(c.size for c in CASES if c.combos == n)
        assert sizes == (["tiny"] if n >= 65535 else ["small"] if n > 1056 else ["disjoint", "multi", "small"] if n in (16, 17, 256) else ["multi", "small"]), (n, sizes)
    assert os.path.getsize(os.path.join(H.GOLDEN, "chain_combo_sweep.npz")) < 500 * 1024


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_inputs_regenerate_with_the_stated_number_of_combinations(case):
    g1, g2, ms, scale = H.combo_input(case)
    z = golden()
    assert H.combo_input_digest(g1, g2, ms, scale) == str(z[case.name + "/digest"]), "the generator of %s has drifted" % case.name
    assert len(g1.path_off) - 1 == case.p1 and len(g2.path_off) - 1 == case.p2
    assert H.count_combinations(g1, g2, ms) == case.combos == int(z[case.name + "/combos"])
    n = ms.n_pairs()
    assert n == int(z[case.name + "/pairs"])
    # sizes: at most one macro-block of 1 024 pairs | at least five | a dozen to a few dozen pairs
    assert {"small": 200 <= n <= 1024, "disjoint": n >= 200, "multi": n >= 4097, "tiny": 12 <= n <= 40}[case.size], n
    if case.size == "disjoint":      # no node on two paths: every match pair lies in one combination
        assert all(len(np.unique(g.path_nodes)) == len(g.path_nodes) for g in (g1, g2))
    assert ((case.name + "/global/dp") in z.files) == (not H.combo_oracle_is_live(case))


@pytest.mark.parametrize("name", RERUN)
def test_oracle_reproduces_the_golden(name):
    case = H.combo_case(name)
    g1, g2, ms, scale = H.combo_input(case)
    z = golden()
    for glob in (True, False):
        pre = "%s/%s/" % (name, "global" if glob else "local")
        chain, dp = po.oracle_chain("affine", g1, g2, ms, scale=scale, want_dp=True, global_anchoring=glob)
        assert np.array_equal(dp[:ms.n_pairs()].view(np.uint32), z[pre + "dp"]) and np.array_equal(chain, z[pre + "chain"]), pre


@pytest.mark.ref
@pytest.mark.parametrize("name", RERUN)
def test_reference_reproduces_the_golden(name):
    case = H.combo_case(name)
    g1, g2, ms, scale = H.combo_input(case)
    z = golden()
    for glob in (True, False):
        pre = "%s/%s/" % (name, "global" if glob else "local")
        chain, _ = po.ref_chain("affine", g1, g2, ms, scale=scale, global_anchoring=glob)
        assert np.array_equal(chain, z[pre + "chain"]), pre
        if (pre + "ref_chain") in z.files:
            assert np.array_equal(z[pre + "ref_chain"], z[pre + "chain"])


@pytest.mark.ref
@pytest.mark.parametrize("case", [c for c in CASES if H.combo_oracle_is_live(c) and c.combos in (1, 2, 8, 9, 16, 17, 256) and H.combo_ref_can_run(c)], ids=repr)
def test_reference_agrees_with_the_live_oracle(case):
    """the cases a GPU test compares with a live oracle run rather than the golden: the oracle's chain is the compiled reference's there too"""
    g1, g2, ms, scale = H.combo_input(case)
    for glob in ((True,) if case.size == "multi" else (True, False)):
        chain = po.oracle_chain("affine", g1, g2, ms, scale=scale, global_anchoring=glob)
        ref, _ = po.ref_chain("affine", g1, g2, ms, scale=scale, global_anchoring=glob)
        assert np.array_equal(ref, chain), (case.name, glob)
