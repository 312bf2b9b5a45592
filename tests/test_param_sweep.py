"""CPU suite: pins the oracles (oracle/popoa_oracle.c, oracle/chain_oracle.cpp) to the reference away from the default scoring — at every
named parameter point of tests/helpers.py (STITCH_SET_NAMES, CHAIN_SETS x CHAIN_SCALES x anchoring).  The GPU sweep (tests/test_gpu_param_sweep.py)
compares the kernels with these oracles, so they are first shown to be the reference there:

* against tests/golden/popoa_param_sweep.npz and chain_param_sweep.npz (results of the compiled reference, tests/golden/make_param_sweep.py);
* live against oracle/_ref on fresh seeds, where it is present.

No parameter set is excluded.  Where the reference itself is undefined — Stitcher::subalign's division by the difference of two equal
neighbouring extends — the NumPW-as-chosen leg has no reference result; there the oracle must refuse (CL_ERR_BAD_GAP_PARAMS), and po_poa with
NumPW 1 / 2 / 3 is compared all the same."""
import os

import numpy as np
import pytest

from centrolign_amd import capi, synth
from oracle import pyoracle as po
from tests import helpers as H

Z = {}


def golden(name):
    if name not in Z:
        Z[name] = np.load(os.path.join(H.GOLDEN, name))
    return Z[name]


def test_parameter_sets_are_valid_and_inside_the_reference_domain():
    """every set is what cl_config_validate accepts, every (set, batch) satisfies the int32 domain condition, 'large' reaches 2^20, the
    random draws are the stored ones, and the sets that leave Stitcher::subalign undefined are exactly the ones with a repeated extend"""
    z = golden("popoa_param_sweep.npz")
    assert tuple(z["set_names"]) == H.STITCH_SET_NAMES
    batches = H.sweep_stitch_batches()
    assert sorted(batches) == list(z["batch_names"])
    undefined = set()
    for name in H.STITCH_SET_NAMES:
        for bname, b in batches.items():
            p = H.stitch_params(name, b)
            term = H.check_stitch_domain(b, p)
            if name == "large":
                assert term >= H.LARGE_TERM_FLOOR
            assert H.alignment_values(p) == z["%s/%s/values" % (name, bname)].tolist()
            assert bool(z["%s/%s/subalign_defined" % (name, bname)][0]) == H.subalign_defined(p)
            if not H.subalign_defined(p):
                undefined.add(name)
    assert {"edit", "free_gaps", "equal_pieces"} <= undefined and not undefined & {"free_mismatch", "near_crossovers", "flat_tail", "large"}
    # near_crossovers: the pieces cross at gap lengths 3 and 21 (open + extend * len: 2 + 5 len = 9 + 2 len, 9 + 2 len = 30 + len)
    o, e = H.STITCH_SETS["near_crossovers"][2:]
    assert (o[1] - o[0]) / (e[0] - e[1]) == pytest.approx(7 / 3) and (o[2] - o[1]) / (e[1] - e[2]) == 21
    for name in H.CHAIN_SETS:
        for glob in (False, True):
            H.chain_params(name, glob)


@pytest.mark.parametrize("name", H.STITCH_SET_NAMES)
def test_popoa_oracle_matches_the_reference_under(name):
    z = golden("popoa_param_sweep.npz")
    for bname, b in H.sweep_stitch_batches().items():
        p = H.stitch_params(name, b)
        pre = "%s/%s/" % (name, bname)
        for npw in (1, 2, 3):
            f = np.full(b.n_problems, npw, np.uint8)
            got = po.oracle_stitch_batch(b, p, force_num_pw=f)
            assert H.sweep_result_diff(got, z, pre + "pw%d." % npw, check_score=True, check_choice=False) is None, (bname, npw)
        if H.subalign_defined(p):
            got = po.oracle_stitch_batch(b, p)
            assert H.sweep_result_diff(got, z, pre + "sub.", check_score=True, check_choice=True) is None, bname
        else:
            with pytest.raises(RuntimeError, match="-2"):
                po.oracle_stitch_batch(b, p)


def test_every_piece_wins_somewhere_under_near_crossovers():
    """the point of near_crossovers: inside the small cases all three pieces are chosen (the NumPW legs give different alignments or scores)"""
    z = golden("popoa_param_sweep.npz")
    differs = {(a, b): False for a, b in ((1, 2), (2, 3))}
    for bname in z["batch_names"]:
        for a, b in differs:
            sa, sb = z["near_crossovers/%s/pw%d.score" % (bname, a)], z["near_crossovers/%s/pw%d.score" % (bname, b)]
            differs[(a, b)] |= bool((sa != sb).any())
    assert all(differs.values()), differs


@pytest.mark.parametrize("name", sorted(H.CHAIN_SETS))
def test_chain_oracle_matches_the_reference_under(name):
    z = golden("chain_param_sweep.npz")
    longest = 0
    for glob in (False, True):
        p = H.chain_params(name, glob)
        for cname, g1, g2, ms in H.sweep_chain_cases():
            pre = "%s/%s/%s/" % (name, "global" if glob else "local", cname)
            got = po.oracle_chain("sparse", g1, g2, ms, params=p, global_anchoring=glob)
            assert np.array_equal(got, z[pre + "sparse"]), pre
            for scale in H.CHAIN_SCALES:
                got, dp = po.oracle_chain("affine", g1, g2, ms, scale=scale, params=p, global_anchoring=glob, want_dp=True)
                assert np.array_equal(got, z[pre + "affine@%g" % scale]), (pre, scale)
                assert not np.isnan(dp).any()
                longest = max(longest, len(got))
    # (two sets make every anchor weight negative — length / sqrt(count) - length^2, and length / sqrt(count) - 4000 — so that the empty chain is the
    # answer: a case of its own; every other set keeps chains of tens of anchors)
    assert (longest == 0) == (name in ("length_1_square", "length_4000_flat")) and (longest == 0 or longest > 10)


@pytest.mark.ref
@pytest.mark.skipif(not po.have_ref(), reason="compiled reference (oracle/_ref) not present")
@pytest.mark.parametrize("name", H.STITCH_SET_NAMES)
def test_popoa_oracle_vs_compiled_reference_live_under(name):
    k = H.STITCH_SET_NAMES.index(name)
    sizes = [(int(a), int(c)) for a, c in np.random.default_rng(900 + k).integers(1, 125, (25, 2))]
    for b in (synth.random_dag_batch(60, seed=400 + k, max_n=80, alphabet=2 + k % 3, allow_empty=False), synth.linear_batch(sizes, seed=500 + k, divergence=0.2),
              synth.near_chain_batch(sizes[:10], seed=600 + k, p_snp=0.08, p_del=0.06, n_long=(0, 1), long_min=22, long_max=40)):
        b.only_deletion_alns[:] = 0
        p = H.stitch_params(name, b)
        for npw in (1, 2, 3):
            f = np.full(b.n_problems, npw, np.uint8)
            ref, _ = po.ref_stitch_batch(b, p, force_num_pw=f)
            got = po.oracle_stitch_batch(b, p, force_num_pw=f)
            assert got.same_as(ref, check_route=False, check_score=False) is None
            n1, n2 = b.sizes()
            m = (n1 > 0) & (n2 > 0)
            assert np.array_equal(got.score[m], ref.score[m])
        if H.subalign_defined(p):
            ref, _ = po.ref_stitch_batch(b, p)
            assert po.oracle_stitch_batch(b, p).same_as(ref, check_score=False, check_route=False) is None


@pytest.mark.ref
@pytest.mark.skipif(not po.have_ref(), reason="compiled reference (oracle/_ref) not present")
@pytest.mark.parametrize("name", sorted(H.CHAIN_SETS))
def test_chain_oracle_vs_compiled_reference_live_under(name):
    from tests.test_extraction import load_stitch_case
    z = np.load(os.path.join(H.GOLDEN, "chain4_30k_merge2.npz"))
    _, graphs, _ = load_stitch_case("stitch4_30k_merge2.npz")
    full = capi.MatchSets(**{k: z["a.ms." + k] for k in capi.MatchSets._DT})
    ms = po.budget_subset(full, 3000, seed=40 + sorted(H.CHAIN_SETS).index(name))
    for glob in (False, True):
        p = H.chain_params(name, glob)
        for algo, scales in (("sparse", (1.0,)), ("affine", H.CHAIN_SCALES)):
            for scale in scales:
                ref, _ = po.ref_chain(algo, graphs[0], graphs[1], ms, scale=scale, params=p, global_anchoring=glob)
                assert np.array_equal(po.oracle_chain(algo, graphs[0], graphs[1], ms, scale=scale, params=p, global_anchoring=glob), ref), (algo, glob, scale)
