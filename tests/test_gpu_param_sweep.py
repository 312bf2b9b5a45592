"""GPU suite: the device kernels at every scoring-parameter point a config file can set (tests/helpers.py: STITCH_SET_NAMES, CHAIN_SETS x
CHAIN_SCALES x anchoring), not only at the defaults.  The oracles these tests compare with are pinned to the compiled reference at the same
points by tests/test_param_sweep.py.  Bit-exact throughout: int32 scores and aligned pairs, float DP values as uint32 patterns.

No parameter set is skipped on the device.  Under the sets with two equal neighbouring extends (edit, free_gaps, equal_pieces, some random
draws) the reference's Stitcher::subalign divides by zero when it chooses NumPW; there the library must answer CL_ERR_BAD_GAP_PARAMS, and the
kernels are compared with NumPW 1, 2 and 3 given — as they are under every set."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from centrolign_amd import capi, synth
from oracle import pyoracle as po
from tests import far_ab_child
from tests import helpers as H
from tests.test_extraction import load_stitch_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FAMILIES = {"general": "popoa_general_kernel", "ring": "popoa_ring_kernel", "sys": "popoa_sys_kernel", "strip": "popoa_strip_kernel", "lane": "popoa_lane_kernel",
            "linear": "popoa_linear_kernel", "quad": "popoa_linear_quad_kernel", "duo": "popoa_linear_duo_kernel", "span": "popoa_linear_span_kernel",
            "persistent": "popoa_chain_persistent_kernel", "narrow": "popoa_narrow_kernel"}
_Z = {}


def golden(name):
    if name not in _Z:
        _Z[name] = np.load(os.path.join(H.GOLDEN, name))
    return _Z[name]


_batches = {}


def family_batches():
    """name -> (batch, environment of the plan): trimmed shapes of the parity tests that between them reach every kernel body.  Kinds that a plan merges into one
    launch (the one-wave chain kinds -> persistent; lane / small systolic launches in plans of 2 048 pairs and more -> narrow) also stand alone in a batch of their own"""
    if _batches:
        return _batches
    rng = np.random.default_rng(3)
    quads = [(a, int(rng.integers(1, 200))) for a in range(1, 17, 3)] + [(int(rng.integers(1, 200)), a) for a in range(2, 17, 3)] + [(16, 16), (1, 1), (16, 900), (3, 3)]
    duos = [(a, int(rng.integers(17, 300))) for a in range(17, 33, 3)] + [(int(rng.integers(17, 300)), a) for a in range(18, 33, 3)] + [(32, 32), (17, 17), (32, 1200)]
    _batches["quads"] = (synth.linear_batch(quads, seed=8, divergence=0.15), {})
    _batches["duos"] = (synth.linear_batch(duos, seed=9, divergence=0.15), {})
    # chains of every geometry (one wave: persistent; linear<W>; span above 1 024 rows), indels long enough to cross the piece boundaries
    chains = [(1, 2), (12, 9), (20, 31), (40, 57), (63, 64), (64, 127), (65, 63), (129, 5), (257, 257), (300, 900), (1024, 70), (1025, 1100), (1100, 1300)]
    dags = synth.sized_dag_batch([(7, 1200), (1200, 7), (60, 900), (63, 64), (200, 800), (800, 200), (255, 256), (1, 300), (500, 500)], seed=5)
    # column predecessors that reach further back than any ring holds: the HBM-plane kernel; dense far bubbles in narrow pairs: the LDS ring
    far = synth.sized_dag_batch([(150, 1500), (100, 1200)], seed=12, extra_edge_p=0.05, skip_max=1500)
    _batches["mixed"] = (capi.StitchBatch.concat([synth.linear_batch(chains, seed=71, divergence=0.2), dags, far, synth.random_dag_batch(40, seed=11, max_n=48, allow_empty=False)]), {})
    _batches["mixed"][0].only_deletion_alns[:] = 0
    # CL_NO_LANE=1: the strips (large branching pairs), the systolic kernel's LDS classes, the ring for what overflows them
    nolane = [synth.sized_dag_batch([(900, 700), (1300, 800), (600, 1500)], seed=33, extra_edge_p=0.05, skip_max=3),
              synth.sized_dag_batch([(150, 2500), (64, 3000), (180, 500), (440, 1200)], seed=11, extra_edge_p=0.15, skip_max=2),
              synth.far_fork_batch([(700, 2000)], seed=71, n_far=3)]
    _batches["no_lane"] = (capi.StitchBatch.concat(nolane), {"CL_NO_LANE": "1"})
    # the planes in HBM: pairs too wide for a ring of eight anti-diagonals in LDS at any NumPW whose forks reach far back in BOTH graphs (no strips, no registers) —
    # random far skips, and long two-branch bubbles in the reference's own topological order (CL_RANK_ORDER=lifo)
    hbm = [synth.sized_dag_batch([(1800, 1900)], seed=12, extra_edge_p=0.05, skip_max=1500),
           synth.near_chain_batch([(1900, 2000)], seed=41, p_snp=0.03, p_del=0.01, n_long=(2, 2), long_min=100, long_max=300, long_other=12)]
    _batches["hbm_planes"] = (capi.StitchBatch.concat(hbm), {"CL_RANK_ORDER": "lifo"})
    # near-chain pairs in registers: one wave, a round of three waves, several rounds; a long bubble -> a saved column
    near = synth.near_chain_batch([(5, 1500), (30, 700), (64, 300), (65, 400), (165, 1200), (300, 330), (420, 418), (700, 30), (90, 90)], seed=5, n_long=(0, 1))
    _batches["near"] = (near, {"CL_LANE_MIN_SWEEP": "0"})
    # a plan of 2 048 pairs and more: lane and small systolic launches as one narrow launch, the one-wave chains as one persistent launch
    head = [synth.near_chain_batch([(40, 600), (600, 50), (130, 500), (190, 400)], seed=40, n_long=(0, 1)), synth.random_dag_batch(120, seed=42, max_n=60, allow_empty=False),
            synth.sized_dag_batch([(120, 300), (200, 700), (40, 60), (60, 900)], seed=43)]
    r2 = np.random.default_rng(46)
    fill = synth.linear_batch([(int(r2.integers(4, 60)), int(r2.integers(4, 120))) for _ in range(2080)], seed=47, divergence=0.15)
    big = capi.StitchBatch.concat(head + [fill])
    big.only_deletion_alns[:] = 0
    _batches["wide_plan"] = (big, {"CL_LANE_MIN_SWEEP": "0"})
    return _batches


def run_plan(ctx, batch, params, force, seen):
    plan = ctx.plan(batch, params, force_num_pw=force)
    plan.execute(); plan.sync()
    for li in plan.launches():
        if li["n_problems"]:
            seen.add(li["kernel"].split("<")[0])
    got = plan.collect()
    plan.destroy()
    return got


@pytest.mark.parametrize("name", H.STITCH_SET_NAMES)
def test_every_kernel_body_under(gpu_ctx, monkeypatch, name):
    """every kernel family runs under the set (asserted from plan.launches(): a set that reroutes everything to one kernel fails here) and gives the oracle's
    scores, pairs, routes and NumPW — NumPW as Stitcher::subalign chooses it where that is defined, and 1, 2, 3 given in any case.
    'large' here is the largest legal set of each batch, which the domain condition ties to the batch's longest pair: a largest term of about 290 000 for the
    quads, 210 000 for the duos, 110 000 for the mixed batch, 70 000 - 90 000 for the strips, the HBM planes, the register kernel and the wide plan.  2^20 is reached
    in test_reference_goldens_on_the_device_under[large] (pairs of at most 245 nodes), through the kernels such pairs take: the one-wave chain kinds in their
    persistent launch, linear<W> and the systolic kernel."""
    seen, by_batch, t0 = set(), {}, time.time()
    for bname, (batch, env) in family_batches().items():
        before = set(seen)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        batch.only_deletion_alns[:] = 0
        p = H.stitch_params(name, batch, require_floor=False)      # ('large': the largest legal values for this batch; 2^20 is reached on the small batches below)
        n = batch.n_problems
        # (the plan of 2 048 pairs and more: every NumPW in one pass, dealt over the pairs in turn)
        legs = [np.full(n, w, np.uint8) for w in (1, 2, 3)] if n < 2048 else [((np.arange(n) + H.STITCH_SET_NAMES.index(name)) % 3 + 1).astype(np.uint8)]
        for f in legs:
            got = run_plan(gpu_ctx, batch, p, f, seen)
            diff = got.same_as(po.oracle_stitch_batch(batch, p, force_num_pw=f))
            assert diff is None, (name, bname, int(f[0]), diff)
        if H.subalign_defined(p):
            got = run_plan(gpu_ctx, batch, p, None, seen)
            diff = got.same_as(po.oracle_stitch_batch(batch, p))
            assert diff is None, (name, bname, "NumPW as chosen", diff)
        else:
            with pytest.raises(capi.ClError) as e:
                gpu_ctx.stitch_batch_align(batch, p)
            assert e.value.code == -2
        for k in env:
            monkeypatch.delenv(k)
        by_batch[bname] = sorted(seen - before)
    missing = [fam for fam, kernel in FAMILIES.items() if kernel not in seen]
    assert not missing, (name, missing, by_batch)
    print("%s: %d kernel names, %.1f s" % (name, len(seen), time.time() - t0))


@pytest.mark.parametrize("name", H.STITCH_SET_NAMES)
def test_reference_goldens_on_the_device_under(gpu_ctx, name):
    """device == compiled reference (tests/golden/popoa_param_sweep.npz), not only device == oracle; here 'large' has its largest term at 2^20 and beyond"""
    z = golden("popoa_param_sweep.npz")
    for bname, b in H.sweep_stitch_batches().items():
        p = H.stitch_params(name, b)
        pre = "%s/%s/" % (name, bname)
        assert H.alignment_values(p) == z[pre + "values"].tolist()
        for npw in (1, 2, 3):
            got = gpu_ctx.po_poa_batch(b, np.full(b.n_problems, npw, np.uint8), p.alignment_params)
            assert H.sweep_result_diff(got, z, pre + "pw%d." % npw, check_score=True, check_choice=False) is None, (bname, npw)
        if H.subalign_defined(p):
            got = gpu_ctx.stitch_batch_align(b, p)
            assert H.sweep_result_diff(got, z, pre + "sub.", check_score=True, check_choice=True) is None, bname
        else:
            with pytest.raises(capi.ClError) as e:
                gpu_ctx.stitch_batch_align(b, p)
            assert e.value.code == -2


@pytest.mark.parametrize("name", ["near_crossovers", "free_gaps"])
def test_second_pass_over_a_resident_batch_gives_the_same_bytes_under(gpu_ctx, name):
    batch = family_batches()["mixed"][0]
    p = H.stitch_params(name, batch, require_floor=False)
    f = ((np.arange(batch.n_problems) % 3) + 1).astype(np.uint8)
    plan = gpu_ctx.plan(batch, p, force_num_pw=f)
    plan.execute(); plan.sync()
    first = plan.collect()
    assert first.same_as(po.oracle_stitch_batch(batch, p, force_num_pw=f)) is None
    for _ in range(2):
        plan.execute(); plan.sync()
        again = plan.collect()
        assert again.same_as(first) is None and np.array_equal(again.score, first.score)
    plan.destroy()


# the chaining DPs --------------------------------------------------------------------------------------------------------------------------
def check_chain(ctx, g1, g2, ms, p, glob, scale, want_affine=None, want_sparse=None):
    got = ctx.chain_sparse_affine(g1, g2, ms, scale=scale, params=p, want_dp=True)
    chain, dp = po.oracle_chain("affine", g1, g2, ms, scale=scale, params=p, want_dp=True, global_anchoring=glob)
    assert np.array_equal(got["dp"].view(np.uint32), dp[:len(got["dp"])].view(np.uint32)), "affine DP values differ"
    assert np.array_equal(got["chain"], chain)
    assert want_affine is None or np.array_equal(got["chain"], want_affine)
    if want_sparse is not False:
        got = ctx.chain_sparse_affine(g1, g2, ms, params=p, want_dp=True, sparse=True)
        chain, dp = po.oracle_chain("sparse", g1, g2, ms, params=p, want_dp=True, global_anchoring=glob)
        assert np.array_equal(got["dp"].view(np.uint32), dp[:len(got["dp"])].view(np.uint32)), "gap-free DP values differ"
        assert np.array_equal(got["chain"], chain)
        assert want_sparse is None or np.array_equal(got["chain"], want_sparse)


@pytest.mark.parametrize("name", sorted(H.CHAIN_SETS))
def test_chaining_kernels_under(gpu_ctx, name):
    """every set x scale x anchoring on the reference's goldens (chain_param_sweep.npz: budgeted subsets of the committed chain4_* match sets), and the committed
    6 000-pair chain4_* inputs whole at one (scale, anchoring) per set and merge in rotation; affine and gap-free: DP values as bit patterns and the chain.
    (The full product runs on the subsets only: the whole inputs are the same graphs and match sets four times as dense, every (scale, anchoring) meets them under
    five or six of the sixteen sets, and the whole product on them would by itself take as long as the rest of this file.)"""
    z = golden("chain_param_sweep.npz")
    cases = H.sweep_chain_cases()
    k = sorted(H.CHAIN_SETS).index(name)
    for glob in (False, True):
        p = H.chain_params(name, glob)
        for cname, g1, g2, ms in cases:
            pre = "%s/%s/%s/" % (name, "global" if glob else "local", cname)
            for i, scale in enumerate(H.CHAIN_SCALES):
                check_chain(gpu_ctx, g1, g2, ms, p, glob, scale, z[pre + "affine@%g" % scale], z[pre + "sparse"] if i == 0 else False)
    # the committed 6 000-pair inputs as they are: every merge, anchoring and scale in rotation over the sets (each combination occurs under several sets)
    for m in range(3):
        zc = np.load(os.path.join(H.GOLDEN, "chain4_30k_merge%d.npz" % m))
        _, graphs, _ = load_stitch_case("stitch4_30k_merge%d.npz" % m)
        ms = capi.MatchSets(**{f: zc["b.ms." + f] for f in capi.MatchSets._DT})
        glob = bool((k + m) % 2)
        check_chain(gpu_ctx, graphs[0], graphs[1], ms, H.chain_params(name, glob), glob, H.CHAIN_SCALES[(k + m) % 3], want_sparse=None)


FAR_MODES = [("auto", {}), ("bb", {"CL_CHAIN_FAR_MODE": "bb"}), ("sweep", {"CL_CHAIN_FAR_MODE": "sweep"}),
             ("per_block", {"CL_CHAIN_NO_FAR_PRUNE": "1", "CL_CHAIN_OLD_WALK": "1", "CL_CHAIN_GROUP_PATH": "0"}), ("lanes8", {"CL_CHAIN_FAR_LANES": "8"}),
             ("group_path", {"CL_CHAIN_GROUP_PATH": "force"})]
FAR_SWITCHES = ("CL_CHAIN_FAR_MODE", "CL_CHAIN_NO_FAR_PRUNE", "CL_CHAIN_OLD_WALK", "CL_CHAIN_FAR_LANES", "CL_CHAIN_GROUP_PATH", "CL_CHAIN_WALK_REDUCE", "CL_CHAIN_WALK2")


def test_far_pass_modes_agree_under_every_chain_set(gpu_ctx, tmp_path):
    """a multi-combination DP in which the far pass really prunes — the root merge of a 4 x 30 kbp MSA, 2 + 2 paths, ~24 k match pairs — under every chain set, in the
    modes auto, bb (the floating-point bound pinned), sweep, per_block (no bound involved), lanes8 and the group-by-group path, each mode in a process of its own that
    runs all the sets: every mode must give per_block's DP values and chain, and the oracle's (computed here).  Anchoring and scale rotate over the sets.
    Under bb the timing log must show the far pass on and no all-pairs sweep for every set: a set under which the host quietly drops the far pass is reported here
    rather than counted as coverage.  Sets for which it is dropped: none on this input.
    What this input does NOT do: with band_pen flipped from the minimum to the maximum over the pieces (tried once on a scratch build) every mode still agreed here;
    that flip is caught by tests/test_gpu_far_modes.py on its 350 k-pair input, at the default parameters only.  An over-eager bound under the other sets would need
    an input that dense to show, which a sweep of this length cannot afford next to an oracle run."""
    seqs = synth.hor_sequences(13, 30000, 4)
    leaves = [capi.leaf_graph(s) for s in seqs]
    scale0 = sum(gpu_ctx.leaf_intrinsic_scale(g) for g in leaves) / 4
    left = gpu_ctx.merge(leaves[0], leaves[1], score_scale=scale0)["fused"]
    right = gpu_ctx.merge(leaves[2], leaves[3], score_scale=scale0)["fused"]
    from bench import relabelled
    g1, g2 = relabelled(left, 5, 6), relabelled(right, 7, 8)
    ms = po.budget_subset(gpu_ctx.find_matches(g1, g2), 24000, seed=6)
    assert ms.n_pairs() > 12000
    names = sorted(H.CHAIN_SETS)
    rows = [H.chain_params(n, global_anchoring=bool(i % 2 == 0)) for i, n in enumerate(names)]
    path = str(tmp_path / "sweep.npz")
    far_ab_child.save_input(path, g1, g2, ms, 0.7, params=rows)
    def oracle_results():      # (on a thread of its own beside the child processes: the oracle is host code and holds no lock of the interpreter)
        out = []
        for p in rows:
            chain, dp = po.oracle_chain("affine", g1, g2, ms, scale=0.7, params=p, want_dp=True, global_anchoring=bool(p.global_anchoring))
            out.append((str(ms.n_pairs()), str(len(chain))) + far_ab_child.digests(dp[:ms.n_pairs()], chain))
        return out
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(1)
    want_future = pool.submit(oracle_results)
    results = {}
    for mode, extra in FAR_MODES:
        env = dict(os.environ, CL_CHAIN_TIMING="1")
        for k in FAR_SWITCHES:
            env.pop(k, None)
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "far_ab_child.py"), path, "affine"], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (mode, r.stdout[-2000:] + r.stderr[-3000:])
        results[mode] = re.findall(r"RESULT pairs=(\d+) anchors=(\d+) dp=(\w+) chain=(\w+)", r.stdout)
        assert len(results[mode]) == len(rows), (mode, r.stdout[-2000:])
        if mode == "bb":
            logs = re.split(r"^PARAMS \d+$", r.stderr, flags=re.M)[1:]
            assert len(logs) == len(rows)
            dropped = [n for n, log in zip(names, logs) if "far pass on" not in log or "all-pairs sweep" in log]
            assert not dropped, "the far pass did not run under %s" % dropped
    want = want_future.result()
    pool.shutdown()
    for mode, got in results.items():
        for n, g, pb, w in zip(names, got, results["per_block"], want):
            assert g == pb, "%s under %s differs from the per-block all-pairs path" % (mode, n)
            assert g == w, "%s under %s differs from the oracle" % (mode, n)


def test_magnitudes_outside_the_int32_domain_are_refused(gpu_ctx):
    """values beyond 2^20 (match, mismatch) / 2^24 (gaps) are taken where the batch's largest pair keeps (n1 + n2 + 2) x largest term below 2^28 — the
    'large' set above — and refused with CL_ERR_INVALID_ARGUMENT where it does not, before anything is launched"""
    b = synth.linear_batch([(300, 300), (5, 5)])
    p = capi.default_stitch_params()
    p.alignment_params.mismatch = 1 << 21
    with pytest.raises(capi.ClError) as e:
        gpu_ctx.stitch_batch_align(b, p)
    assert e.value.code == -1 and "too large" in str(e.value)
    p = capi.default_stitch_params()
    p.alignment_params.gap_open[:] = [60, 800, 1 << 25]
    with pytest.raises(capi.ClError) as e:
        gpu_ctx.stitch_batch_align(b, p)
    assert e.value.code == -1 and "too large" in str(e.value)
    small = synth.linear_batch([(20, 30), (5, 5)])
    p = capi.default_stitch_params()
    p.alignment_params.mismatch = 1 << 21
    H.check_stitch_domain(small, p)
    assert gpu_ctx.stitch_batch_align(small, p).same_as(po.oracle_stitch_batch(small, p)) is None
