"""The anti-diagonal kernels of the stitch path, popoa_general_kernel<NPW, BLOCK> and popoa_ring_kernel<NPW, BLOCK> (popoa_kernels.hip), in every instantiation, LDS
class and ring mode, bit for bit against the oracle.

They are the kernels of last resort: whatever the register, systolic, strip and chain kernels refuse ends up on them, and cl_stitch_plan_collect runs every strip pair
that reports status 9 again on popoa_general_kernel<npw, 1024>.  With the default routing almost no shape reaches them, so the tests here send ordinary shapes there with
the routing hooks that plan creation reads per plan (read_pack_switches):
    A = CL_FORCE_GENERAL=1 CL_NO_SYS=1              the LDS ring where choose_ring takes the pair, else planes in HBM
    B = A + CL_NO_RING=1                            planes in HBM only
test_the_hooks_are_read_per_plan keeps all of this from silently testing the default route; every run asserts that nothing but the two kernels was launched, and that
the launches are the ones choose_ring's rule (restated below from the batch alone) predicts: kernel, NumPW, workgroup size, LDS class and LDS bytes.

What the shapes are for:
  * the workgroup size is 64 / 256 / 1 024 threads for a shorter side + 1 of <= 64 / <= 256 / above: shorter sides 63 | 64 and 255 | 256 in both orientations, and
    1 023 | 1 024 — 1 025 cells per anti-diagonal is the only case in which a workgroup of 1 024 goes round its `t += BLOCK` / `a += BLOCK` loop twice;
  * pairs of one and two nodes, one node against 300;
  * chains (every read one rank back: a ring of depth 4 covers them), random DAGs with short skip edges, several sources and sinks and in-degrees beyond two;
  * a ring above 64 KB that covers every read: the chain pair 1 023 x 1 100 at NumPW 1 (91 KB); at NumPW 2 and 3 the same pair overflows 128 KB and takes the HBM
    planes at 1 024 threads without hook B.  HBM planes at 64 threads without hook B: 40 x 4 500 at NumPW 3, whose topology alone is 130 KB;
  * the DRAINED ring (the ring does not cover every read: far reads go to the HBM planes, which are drained every depth/2 anti-diagonals): explicit chains with skip
    edges of 6 7 8 9 15 16 17 31 32 33 63 64 65 127 128 129 ranks in both graphs.  The ring depth is a power of two between 8 and 128 here, so whatever it is, the insertion
    reads (distance = a skip of graph 1), the deletion reads (a skip of graph 2) and the diagonal reads (the sum of one of each, the chain edge's 1 included: 6 + 1, 7 + 1,
    7 + 8, 15 + 16, 31 + 33, ...) lie at depth - 1, depth and depth + 1.  Both orientations, because a graph of 63 nodes holds no skip of 63 and more.  The same pairs with second sources in mid-graph: a
    source's boundary read counts into the span, so the ring's `need` exceeds every real ring read;
  * three pairs built for one term of the recurrence each, because random inputs do not make it decide anything (each was found by changing that term in a scratch
    build and seeing every other test here pass): a many-predecessor node whose last read is at exactly the ring depth (fan_in_batch), a leading gap through a bubble
    (leading_gap_batch: the boundary pre-pass's shortcut), two gaps in a row at a source (two_gaps_batch: the source's term of I and D in interior cells);
  * every NumPW (force_num_pw) with the default scores, the tie-heavy ones (match = mismatch = 1: traceback_wave's equality tests on planes these kernels wrote) and
    `pieces`, under which gaps of 1, 8 and 45 nodes are cheapest in the first, second and third piece;
  * a resident plan executed three times: the same bytes each time;
  * the fallback launch of cl_stitch_plan_collect, popoa_general_kernel<npw, 1024> on pairs whose anti-diagonals are far narrower than the workgroup.

What this file cannot show is the drain cadence.  A drained ring whose __syncthreads() every depth/2 anti-diagonals were weakened to the LDS-only barrier is a race (a far
read of the HBM planes could overtake the store it needs); it may still give the oracle's bytes on every run, and no test here claims to catch it."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from centrolign_amd import capi, synth
from oracle import pyoracle as po
from tests import helpers as H
from tests.test_gpu_lane_cells import _graph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOK_NAMES = ("CL_FORCE_GENERAL", "CL_NO_SYS", "CL_NO_RING", "CL_NO_STRIP", "CL_NO_LANE")
HOOKS = {"": {}, "A": dict(CL_FORCE_GENERAL="1", CL_NO_SYS="1"), "B": dict(CL_FORCE_GENERAL="1", CL_NO_SYS="1", CL_NO_RING="1")}
RING, GENERAL = "popoa_ring_kernel", "popoa_general_kernel"
RING_LDS_BYTES = 128 * 1024      # kRingLdsBytes (cl_stitch_plan_api.cpp)
LDS_SPLIT = 64 * 1024            # form_general_groups: rings above it are launches of their own (one workgroup per compute unit)


def _set_hooks(monkeypatch, which, order="auto"):
    for name in HOOK_NAMES + ("CL_RANK_ORDER", "CL_LANE_MIN_SWEEP"):
        monkeypatch.delenv(name, raising=False)
    for name, value in HOOKS[which].items():
        monkeypatch.setenv(name, value)
    if order != "auto":
        monkeypatch.setenv("CL_RANK_ORDER", order)


# ---- choose_ring and form_general_groups, restated from the batch alone ------------------------------------------------------------------------------
def ring_rule(batch, k, npw, order="auto"):
    """what choose_ring decides for pair k at NumPW npw.  With w = min(n1, n2) + 1: per_diag = w (1 + 2 npw) 4 bytes; topo = (n1 + n2) 8 + edges 4 +
    (n1 + n2 + 2)(1 + npw) 4 + 16 bytes; need = span1 + span2 + 1 anti-diagonals (span: how many ranks back a node reads, a source's boundary read included); the depth
    doubles while it is below need and 2 depth per_diag + topo <= 128 KB; taken if it fits and (depth >= 8 or covers every read).  order: CL_RANK_ORDER of the plan"""
    n, span, edges, dist = [0, 0], [0, 0], 0, [set(), set()]
    for s in (0, 1):
        side = batch.side[s]
        b0, b1 = int(side.node_off[k]), int(side.node_off[k + 1])
        n[s] = b1 - b0
        if not n[s]:
            return None      # a pure deletion: no device launch
        rank = np.empty(n[s], np.int64)
        rank[capi.stitch_rank_order(batch, k, s, order)[0].astype(np.int64)] = np.arange(n[s])
        off = side.prev_off[b0:b1 + 1].astype(np.int64)
        heads = np.repeat(np.arange(n[s]), np.diff(off))
        tails = side.prev_idx[int(off[0]):int(off[-1])].astype(np.int64)
        if len(tails):
            span[s] = int((rank[heads] - rank[tails]).max())
            dist[s] = set((rank[heads] - rank[tails]).tolist())
        src = side.src_idx[int(side.src_off[k]):int(side.src_off[k + 1])].astype(np.int64)
        span[s] = max(span[s], int(rank[src].max()) + 1)
        edges += len(tails)
    w = min(n) + 1
    per_diag = w * (1 + 2 * npw) * 4
    topo = (n[0] + n[1]) * 8 + edges * 4 + (n[0] + n[1] + 2) * (1 + npw) * 4 + 16
    need = span[0] + span[1] + 1
    depth = 1
    while depth < need and 2 * depth * per_diag + topo <= RING_LDS_BYTES and depth < 16384:
        depth *= 2
    taken = depth * per_diag + topo <= RING_LDS_BYTES and (depth >= 8 or depth >= need)
    return dict(n=tuple(n), taken=taken, depth=depth, need=need, per_diag=per_diag, topo=topo, lds=depth * per_diag + topo if taken else 0,
                block=64 if w <= 64 else 256 if w <= 256 else 1024, drained=taken and depth < need, dist=dist)


def _lds_class(lds):
    return 0 if lds == 0 else 1 if lds <= LDS_SPLIT else 2


def predicted_launches(batch, npw, hook, order="auto"):
    """{(kernel, NumPW, workgroup size, LDS class): dynamic LDS of the launch} under hook A or B"""
    out = {}
    for k in range(batch.n_problems):
        r = ring_rule(batch, k, int(npw[k]), order)
        if r is None:
            continue
        lds = r["lds"] if hook == "A" else 0
        key = (RING if lds else GENERAL, int(npw[k]), r["block"], _lds_class(lds))
        out[key] = max(out.get(key, 0), lds)
    return out


def planned_launches(plan):
    out = {}
    for li in plan.launches():
        if not li["n_problems"]:
            continue
        m = re.fullmatch(r"(popoa_\w+)<(\d), (\d+)>", li["kernel"])
        assert m and m.group(1) in (RING, GENERAL), "a launch of another kernel: %s" % li["kernel"]
        key = (m.group(1), int(m.group(2)), int(m.group(3)), _lds_class(li["lds_bytes"]))
        assert key not in out, "two launches of one class: %r" % (key,)
        out[key] = li["lds_bytes"]
    return out


# ---- the batches -----------------------------------------------------------------------------------------------------------------------------------------
BLOCK_EDGES = [(63, 80), (80, 63), (64, 80), (255, 300), (300, 256), (1023, 1100), (1100, 1024)]
DEGENERATE = [(1, 1), (1, 2), (2, 1), (1, 300), (300, 1)]
SKIPS = (6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
DRAINED = [(63, 400), (200, 420), (300, 420)]      # ring depths by the rule at NumPW 3: 64, 16, 8; (63, 400) at NumPW 1: 128


def skip_graph(n, seed, srcs=()):
    """a chain of n nodes with one skip edge of every length in SKIPS that fits (a skip of s ranks: _graph's dels = (p, s - 1), from position p - 1 to p + s - 1), spread over
    the chain; where some do not fit, also the longest that does (n - 1 ranks, first node to last), so that the short graph of a pair still adds to the ring's `need`
    (and 62 + 65 = 127 is the diagonal read at depth - 1 of the 63-node graph's ring of 128)"""
    lengths = [s for s in SKIPS if s <= n - 1]
    if len(lengths) < len(SKIPS):
        lengths.append(n - 1)
    dels = [(1 + (41 * i) % (n - s), s - 1) for i, s in enumerate(lengths)]
    assert all(1 <= p and p + length <= n - 1 for p, length in dels)
    return _graph(n, seed, dels=dels, srcs=srcs)[0], lengths


def drained_batch(sources):
    pairs, skips = [], []
    for i, (n1, n2) in enumerate(DRAINED):
        (g1, s1), (g2, s2) = (skip_graph(n, 100 + 2 * i + j, srcs=[n // 3, n // 2 + 3] if sources else ()) for j, n in enumerate((n1, n2)))
        pairs += [(g1, g2), (g2, g1)]
        skips += [(s1, s2), (s2, s1)]
    return H.batch_from_graphs(pairs), skips


def _chain_graph(labels, extra_edges=(), sources=(0,)):
    """a chain over the labels with further edges behind the chain's own in every predecessor list, in the order given"""
    n = len(labels)
    return dict(labels=[int(x) for x in labels], edges=[(i, i + 1) for i in range(n - 1)] + list(extra_edges), sources=list(sources), sinks=[n - 1])


# fan-in nodes of the row graph: (rows, [(rank a of the node, D)]): predecessors 1, 2, ..., D ranks back, the one at D last in its list
FAN_IN = [(200, [(72, 16), (140, 32)]), (300, [(68, 8), (136, 16), (200, 32)])]


def fan_in_batch():
    """An insertion read at exactly the ring depth, in a cell the best alignment passes through, by a lane that has D - 1 predecessors to work through first.
    The slot of anti-diagonal d - depth is the one anti-diagonal d is being written to, so a kernel that took the read at distance == depth from the ring would read
    a slot that another lane overwrites during this very anti-diagonal: the node's rank a lies in the wave after the one of rank a - D, whose lanes (one predecessor
    each) have written long before the last of the D reads.  (A race all the same: such a kernel is wrong, but a run need not show it.)
    Graph 1: a chain with, for every (a, D), edges into rank a from 2 .. D ranks back.  Graph 2: the same sequence without the ranks a - D + 1 .. a + 2 and with a
    random tail: the best alignment takes the longest edge into rank a and leaves ranks a, a + 1, a + 2 unaligned — the insertion state at (a, column of rank a - D),
    opened from the cell D ranks back.  Ring depths by the rule: 200 rows 32 / 16 / 16 at NumPW 1 / 2 / 3, 300 rows 32 / 16 / 8"""
    rng = np.random.default_rng(530)
    pairs = []
    for rows, fans in FAN_IN:
        lab = rng.integers(1, 5, size=rows)
        keep = np.ones(rows, bool)
        extra = []
        for a, depth in fans:
            t = a - 1                                     # node id = rank - 1 in a chain
            extra += [(t - j, t) for j in range(2, depth + 1)]
            keep[t - depth + 1:t + 3] = False
        g1 = _chain_graph(lab, extra)
        g2 = _chain_graph(np.concatenate([lab[keep], rng.integers(1, 5, size=420 - int(keep.sum()))]), [(i, i + 40) for i in (20, 130, 250)])
        pairs += [(g1, g2), (g2, g1)]
    return H.batch_from_graphs(pairs)


def leading_gap_batch():
    """The boundary column and row are 1-D recurrences that popoa_ring_kernel does up front, with a shortcut for a node whose one predecessor is the rank before it.
    Here the best alignment begins with a gap that runs through a bubble whose branches have five nodes and one: the gap's cost at the node behind the bubble is right
    only if the short branch's node (one predecessor, the fork, which is NOT the rank before it when a node of the long branch is ranked in between) reads the fork.
    The fork's edges in both orders (the reference's topological order takes the branch of the LAST edge first), the bubble in either graph;
    test_the_crafted_pairs_are_what_they_are_for checks in rank space that the shortcut, taken by every node with one predecessor, would make the gap dearer"""
    rng = np.random.default_rng(531)
    pairs = []
    for short_first in (False, True):
        common = rng.integers(1, 4, size=25)             # labels 1-3; everything in front of it is 4 and aligns with nothing
        long_ids, short_id = (list(range(2, 7)), 1) if short_first else (list(range(1, 6)), 6)
        m = 7
        fork = [(0, short_id), (0, long_ids[0])] if short_first else [(0, long_ids[0]), (0, short_id)]
        edges = fork + [(long_ids[i], long_ids[i + 1]) for i in range(4)] + [(long_ids[4], m), (short_id, m)]
        n = m + 1 + 6 + len(common)
        edges += [(i, i + 1) for i in range(m, n - 1)]
        g1 = dict(labels=[4] * (m + 7) + [int(x) for x in common], edges=edges, sources=[0], sinks=[n - 1])
        other = common.copy()
        other[11] = other[11] % 3 + 1
        g2 = _chain_graph(other)
        pairs += [(g1, g2), (g2, g1)]
    return H.batch_from_graphs(pairs)


def two_gaps_batch():
    """The best alignment begins with a gap in one graph and then a gap in the other, at a source (the first one, or a second one in mid-graph).  Either order of the
    two gaps scores the same, and the traceback's test order (I_0, D_0, I_1, D_1, ...) decides: with a long gap (a later piece under the scoring of `pieces`) in one
    graph and a one-node gap (piece 0) in the other, the one-node gap is found first — but only if the cell behind both gaps holds it, which is the term `source:
    M(boundary) - open - extend` of I and D in the interior.  Without that term the cell's M and the score stay right (the other order gives them) and the alignment
    comes out in the other order"""
    pairs = []
    rng = np.random.default_rng(532)
    for long_gap in (8, 45):
        common = rng.integers(1, 3, size=30)
        a = _chain_graph([3] * long_gap + [int(x) for x in common])
        b = _chain_graph([4] + [int(x) for x in common])
        c = _chain_graph([4] * 7 + [int(x) for x in common], sources=(0, 6))     # a second source in mid-graph: the same alignment, begun there
        pairs += [(a, b), (b, a), (a, c), (c, a)]
    return H.batch_from_graphs(pairs)


def _sized(sizes, **kw):
    b = synth.sized_dag_batch(sizes, **kw)
    n1, n2 = b.sizes()
    assert [(int(x), int(y)) for x, y in zip(n1, n2)] == sizes
    return b


GROUPS = {
    "edges_chains": lambda: synth.linear_batch(BLOCK_EDGES, seed=501),
    "edges_dags": lambda: _sized(BLOCK_EDGES, seed=502),
    "edges_dense_dags": lambda: _sized(BLOCK_EDGES, seed=503, extra_edge_p=0.4, skip_max=6, alphabet=2),
    "degenerate": lambda: capi.StitchBatch.concat([synth.linear_batch(DEGENERATE, seed=504), _sized(DEGENERATE, seed=505),
                                                   _sized(DEGENERATE, seed=506, extra_edge_p=0.4, skip_max=6, alphabet=2)]),
    "random_dags": lambda: synth.random_dag_batch(300, seed=507, max_n=60),
    "hbm_at_64_threads": lambda: _sized([(40, 4500), (4500, 40)], seed=508),
    "drained": lambda: drained_batch(False)[0],
    "drained_sources": lambda: drained_batch(True)[0],
    "fan_in_at_the_ring_depth": fan_in_batch,
    "leading_gap_through_a_bubble": leading_gap_batch,
    "two_gaps_at_a_source": two_gaps_batch,
}
# the packer's own rank order puts a second source first, and what is far is then the edge out of it; in the reference's order the source sits in mid-graph next to
# the node it feeds, and what is far is its boundary read (tests/test_gpu_lane_cells.py)
RANK_ORDER = {"drained_sources": "lifo"}
_batches, _oracle = {}, {}
_seen = {}       # (group, hook, NumPW) -> planned_launches of the group's plan (from test_against_the_oracle, which executed it, where that test ran first)


def _batch(group):
    if group not in _batches:
        _batches[group] = GROUPS[group]()
    return _batches[group]


def _params(which):
    """default; ties: match = mismatch = 1; pieces: a mismatch costs more than any two gaps, and the cheapest piece of a gap of 1, 8 and 45 nodes is the first (5 against 12
    and 41), the second (26 against 33 and 48) and the third (85 against 100 and 181)"""
    if which == "pieces":
        p = capi.default_stitch_params()
        p.alignment_params = capi.make_align_params(2, 100, [1, 10, 40], [4, 2, 1])
        return p
    return H.tie_params() if which == "ties" else capi.default_stitch_params()


def _want(group, npw, which):
    key = (group, npw, which)
    if key not in _oracle:
        b = _batch(group)
        _oracle[key] = po.oracle_stitch_batch(b, params=_params(which), force_num_pw=np.full(b.n_problems, npw, np.uint8))
    return _oracle[key]


def _same_bytes(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("aln_off", "pairs", "score", "route", "num_pw"))


def _plan(gpu_ctx, monkeypatch, batch, hook, npw, params=None, order="auto"):
    """a plan under the hook, with its launches checked against the rule"""
    _set_hooks(monkeypatch, hook, order)
    plan = gpu_ctx.plan(batch, params=params, force_num_pw=npw)
    got, want = planned_launches(plan), predicted_launches(batch, npw, hook, order)
    assert got == want, "hook %s: the plan's launches %r are not what choose_ring's rule predicts, %r" % (hook, got, want)
    return plan, got


# ---- (a) the hooks are live ------------------------------------------------------------------------------------------------------------------------------
def test_the_hooks_are_read_per_plan(gpu_ctx, monkeypatch):
    """one process, one small batch, three plans (none executed): no hook -> the register, systolic and chain kernels (the chain pairs of at most 64 rows in the
    persistent one-wave launch); A -> nothing but the two anti-diagonal kernels,
    the ring among them; B -> popoa_general_kernel alone.  Every other test of this file relies on it"""
    b = capi.StitchBatch.concat([synth.near_chain_batch([(150, 500)], seed=510), synth.random_dag_batch(20, seed=511, max_n=30, allow_empty=False),
                                 synth.linear_batch([(10, 12), (100, 120), (300, 280)], seed=512)])
    f = np.ones(b.n_problems, np.uint8)
    names = {}
    for hook in ("", "A", "B", ""):      # (and back: unsetting them is seen as well)
        _set_hooks(monkeypatch, hook)
        plan = gpu_ctx.plan(b, force_num_pw=f)
        now = sorted(li["kernel"] for li in plan.launches() if li["n_problems"])
        plan.destroy()
        assert names.setdefault(hook, now) == now, (hook, names[hook], now)
    assert names[""] and all(n.startswith(("popoa_lane_kernel", "popoa_sys_kernel", "popoa_linear", "popoa_chain_persistent_kernel")) for n in names[""]), names[""]
    assert any(n.startswith("popoa_linear") for n in names[""]) and any(n.startswith(("popoa_lane_kernel", "popoa_sys_kernel")) for n in names[""]), names[""]
    assert all(n.startswith((RING, GENERAL)) for n in names["A"]) and any(n.startswith(RING) for n in names["A"]), names["A"]
    assert names["B"] and all(n.startswith(GENERAL) for n in names["B"]), names["B"]


# ---- (b) - (d) every group against the oracle, every NumPW, both hooks, both scorings --------------------------------------------------------------
@pytest.mark.parametrize("scoring", ["default", "ties", "pieces"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_against_the_oracle(gpu_ctx, monkeypatch, group, scoring):
    b = _batch(group)
    for npw in (1, 2, 3):
        f = np.full(b.n_problems, npw, np.uint8)
        want = _want(group, npw, scoring)
        for hook in ("A", "B"):
            plan, launches = _plan(gpu_ctx, monkeypatch, b, hook, f, _params(scoring), RANK_ORDER.get(group, "auto"))
            plan.execute(); plan.sync()
            diff = plan.collect().same_as(want)
            plan.destroy()
            assert diff is None, "%s, NumPW %d, hook %s, %s scores: %s" % (group, npw, hook, scoring, diff)
            _seen[(group, hook, npw)] = launches


def test_the_shapes_are_what_they_are_for():
    """host only: the rule gives the named shapes the classes and ring modes they were chosen for (the plans of the other tests are checked against the same rule)"""
    chains = _batch("edges_chains")
    big = [k for k, s in enumerate(BLOCK_EDGES) if min(s) >= 1023]
    for k in big:
        r = ring_rule(chains, k, 1)      # a ring above 64 KB that covers every read
        assert r["taken"] and not r["drained"] and r["depth"] == 4 and r["block"] == 1024 and r["lds"] > LDS_SPLIT, r
        for npw in (2, 3):               # ... which at NumPW 2 and 3 overflows 128 KB: planes in HBM at 1 024 threads without hook B
            r = ring_rule(chains, k, npw)
            assert not r["taken"] and r["block"] == 1024, r
    for k in range(2):                   # the topology alone leaves no room for a ring of two anti-diagonals: planes in HBM at 64 threads without hook B
        r = ring_rule(_batch("hbm_at_64_threads"), k, 3)
        assert not r["taken"] and r["block"] == 64 and r["topo"] + 2 * r["per_diag"] > RING_LDS_BYTES, r
    for sources in (False, True):
        b, skips = drained_batch(sources)
        depths = {}
        for k in range(b.n_problems):
            for npw in (1, 2, 3):
                r = ring_rule(b, k, npw, "lifo" if sources else "auto")
                # no ring could cover every read, so the drained mode runs
                assert r["taken"] and r["drained"] and r["need"] * r["per_diag"] > RING_LDS_BYTES, (k, npw, r)
                depths[(min(r["n"]), npw)] = d = r["depth"]
                far = max(r["dist"][0]) + max(r["dist"][1])
                if sources:              # a source's boundary read makes `need` larger than any ring read
                    assert r["need"] > far + 1 and far > d, (k, npw, r["need"], far, d)
                    continue
                # reads on both sides of the ring depth, in rank space: the insertion reads where graph 1 is the longer graph (k odd), the deletion reads where
                # graph 2 is (k even), the diagonal reads in both
                assert r["need"] == far + 1 and r["dist"][0] == set(skips[k][0]) | {1} and r["dist"][1] == set(skips[k][1]) | {1}, (k, npw)
                assert {d - 1, d, d + 1} <= r["dist"][1 - k % 2], (k, npw, d)
                assert {d - 1, d, d + 1} <= {x + y for x in r["dist"][0] for y in r["dist"][1]}, (k, npw, d)
        if not sources:
            assert (depths[(63, 3)], depths[(63, 1)], depths[(200, 3)], depths[(300, 3)]) == (64, 128, 16, 8), depths


def _gap_lengths(batch, k, s, shortcut_for_every_single_predecessor):
    """nodes in the shortest gap from a source to every node of graph s, by rank, as the boundary pre-pass of popoa_ring_kernel computes it: a node whose one predecessor
    is the rank before it takes that rank's value from a register.  With the flag: what comes out if every node with one predecessor did so"""
    side = batch.side[s]
    b0, b1 = int(side.node_off[k]), int(side.node_off[k + 1])
    order = capi.stitch_rank_order(batch, k, s)[0].astype(np.int64)
    rank = np.empty(b1 - b0, np.int64)
    rank[order] = np.arange(b1 - b0)
    sources = set(int(x) for x in side.src_idx[int(side.src_off[k]):int(side.src_off[k + 1])])
    out = []
    for r, v in enumerate(order):
        preds = [int(rank[u]) for u in side.prev_idx[int(side.prev_off[b0 + v]):int(side.prev_off[b0 + v + 1])]]
        if len(preds) == 1 and (shortcut_for_every_single_predecessor or preds[0] == r - 1):
            preds = [r - 1]
        out.append(min([1 + out[q] if q >= 0 else 10 ** 9 for q in preds] + ([1] if int(v) in sources else [])))
    return np.array(out)[rank]      # by node id


def test_the_crafted_pairs_are_what_they_are_for():
    """host only: the fan-in nodes read at the ring depth the rule gives, and the oracle's alignments begin the way the cases were built for"""
    b = _batch("fan_in_at_the_ring_depth")
    for i, (rows, fans) in enumerate(FAN_IN):
        for k in (2 * i, 2 * i + 1):
            depths = {npw: ring_rule(b, k, npw) for npw in (1, 2, 3)}
            assert all(r["drained"] and r["block"] == (256 if rows == 200 else 1024) for r in depths.values()), (k, depths)
            assert {r["depth"] for r in depths.values()} == {d for _, d in fans}, (k, depths)
        want = _want("fan_in_at_the_ring_depth", 1, "default")
        aln = want.alignment(2 * i)
        for a, depth in fans:      # rank a - D aligned, ranks a .. a + 2 against a gap, nothing in between: the edge of D ranks was taken
            rows_in = [int(x) for x in aln[:, 0] if x != capi.CL_GAP]
            at = rows_in.index(a - 1)
            assert rows_in[at - 1] == a - 1 - depth and all(aln[j, 1] == capi.CL_GAP for j in range(len(aln)) if aln[j, 0] != capi.CL_GAP and a - 1 <= aln[j, 0] <= a + 1), (rows, a, depth)
    gaps = _want("leading_gap_through_a_bubble", 1, "default")
    for k in range(0, 4, 2):       # the gap in front runs fork, short branch, node behind the bubble, six more: nine nodes
        aln = gaps.alignment(k)
        assert all(aln[j, 1] == capi.CL_GAP for j in range(9)) and aln[9, 1] != capi.CL_GAP, (k, aln[:12])
        for kk, s in ((k, 0), (k + 1, 1)):      # ... and its last node (id 13) is the ninth; with the short branch ranked behind a node of the long one (pairs 2 and 3)
            right, shortcut = (_gap_lengths(_batch("leading_gap_through_a_bubble"), kk, s, flag)[13] for flag in (False, True))     # only if its node reads the fork
            assert right == 9 and (shortcut > 9 if k == 2 else shortcut == 9), (kk, s, right, shortcut)
    two = _want("two_gaps_at_a_source", 3, "pieces")
    for k in range(0, 8, 4):       # (a, b): the long gap of graph 1 comes out first, then the one node of graph 2
        aln = two.alignment(k)
        n_long = 8 if k == 0 else 45
        assert all(aln[j, 1] == capi.CL_GAP for j in range(n_long)) and aln[n_long, 0] == capi.CL_GAP and aln[n_long + 1, 0] != capi.CL_GAP, (k, aln[:n_long + 3])


# ---- (e) a resident plan, executed three times ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hook", ["A", "B"])
def test_a_resident_plan_gives_the_same_bytes_every_time(gpu_ctx, monkeypatch, hook):
    small = [k for k, s in enumerate(BLOCK_EDGES) if max(s) <= 300]
    b = capi.StitchBatch.concat([_batch("edges_dense_dags").subset(small), _batch("drained").subset([0, 3, 4]), _batch("drained_sources").subset([1, 2]),
                                 _batch("random_dags").subset(np.arange(60)), _batch("edges_chains").subset(small)])
    f = (np.arange(b.n_problems) % 3 + 1).astype(np.uint8)
    want = po.oracle_stitch_batch(b, force_num_pw=f)
    plan, _ = _plan(gpu_ctx, monkeypatch, b, hook, f)
    first = None
    for _ in range(3):
        plan.execute(); plan.sync()
        got = plan.collect()
        assert got.same_as(want) is None
        first = first or got
        assert _same_bytes(got, first)
    plan.destroy()


# ---- (f) the fallback launch ---------------------------------------------------------------------------------------------------------------------------------
FALLBACK_SIZES = [(191, 530), (530, 191), (200, 500), (500, 200), (255, 400), (400, 256), (700, 720), (720, 700)]


def test_the_fallback_launch_on_narrow_pairs():
    """cl_stitch_plan_collect runs a pair that reports status 9 again on popoa_general_kernel<npw, 1024>, whatever its size.  CL_STRIP_DEBUG_FAIL=1 (read once per
    process, hence the one child) makes every second pair of popoa_strip_kernel report it.  The switch does not reach popoa_lane_kernel, so these are strip pairs, under
    CL_NO_LANE=1 CL_NO_SYS=1 and at the smallest sizes fit_strips takes (192 rows with the boundary row, 100 000 cells) upwards: anti-diagonals of 192 to 701 cells on
    a workgroup of 1 024, at every NumPW"""
    code = ("import sys, json; sys.path.insert(0, %r)\n"
            "import numpy as np\n"
            "from centrolign_amd import capi, synth\n"
            "from oracle import pyoracle as po\n"
            "ctx = capi.Context(0)\n"
            "b = synth.sized_dag_batch(%r, seed=520, extra_edge_p=0.05, skip_max=3)\n"
            "out = []\n"
            "for npw in (1, 2, 3):\n"
            "    f = np.full(b.n_problems, npw, np.uint8)\n"
            "    plan = ctx.plan(b, force_num_pw=f)\n"
            "    strips = all(li['kernel'].startswith('popoa_strip_kernel') for li in plan.launches() if li['n_problems'])\n"
            "    plan.execute(); plan.sync(); got = plan.collect()\n"
            "    out.append(dict(npw=npw, strips=strips, same=got.same_as(po.oracle_stitch_batch(b, force_num_pw=f)) is None, fallbacks=plan.stats()['n_strip_fallbacks']))\n"
            "    plan.destroy()\n"
            "print(json.dumps(out))\n" % (ROOT, FALLBACK_SIZES))
    env = dict(os.environ, CL_STRIP_DEBUG_FAIL="1", CL_NO_LANE="1", CL_NO_SYS="1")
    for name in ("CL_FORCE_GENERAL", "CL_NO_STRIP", "CL_NO_RING"):
        env.pop(name, None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x["npw"] for x in res] == [1, 2, 3]
    for x in res:
        # every pair is a strip pair, so the pairs 1, 3, 5, 7 came back from the fallback launch: shorter sides 191, 200, 256 and 700
        assert x["same"] and x["strips"] and x["fallbacks"] == len(FALLBACK_SIZES) // 2 >= 2, res


# ---- (b) every instantiation and LDS class ----------------------------------------------------------------------------------------------------------------
def test_every_instantiation_and_lds_class(gpu_ctx, monkeypatch):
    """over the batches of test_against_the_oracle (planned again here where that test did not run before this one): all nine popoa_general_kernel<NPW, BLOCK>, all
    nine popoa_ring_kernel<NPW, BLOCK>, and for every BLOCK a ring of at most 64 KB and one above (above 64 KB a launch has one workgroup per compute unit).
    No class turned out to be unreachable.  Prints the set (pytest -s)"""
    classes = {}
    for group in sorted(GROUPS):
        b = _batch(group)
        for npw in (1, 2, 3):
            for hook in ("A", "B"):
                if (group, hook, npw) not in _seen:
                    plan, launches = _plan(gpu_ctx, monkeypatch, b, hook, np.full(b.n_problems, npw, np.uint8), order=RANK_ORDER.get(group, "auto"))
                    plan.destroy()
                    _seen[(group, hook, npw)] = launches
                for key, lds in _seen[(group, hook, npw)].items():
                    classes.setdefault(key, []).append((group, hook, lds))
    print("\nlaunch classes (kernel, NumPW, BLOCK, LDS class 0 none / 1 <= 64 KB / 2 above): groups under a hook, largest dynamic LDS")
    for key in sorted(classes):
        print("  %-22s NumPW %d  BLOCK %4d  class %d   %6d bytes   %s" % (key + (max(x[2] for x in classes[key]), " ".join(sorted({"%s/%s" % x[:2] for x in classes[key]})))))
    for block in (64, 256, 1024):
        for npw in (1, 2, 3):
            assert (GENERAL, npw, block, 0) in classes, (GENERAL, npw, block)
            assert any((RING, npw, block, c) in classes for c in (1, 2)), (RING, npw, block)
        for c in (1, 2):
            assert any((RING, npw, block, c) in classes for npw in (1, 2, 3)), (RING, block, c)
    # without hook B: planes in HBM at 1 024 threads (the chain pairs of 1 023 and 1 024 at NumPW 2, 3) and at 64 threads (40 x 4 500 at NumPW 3)
    assert (GENERAL, 2, 1024, 0) in _seen[("edges_chains", "A", 2)] and (GENERAL, 3, 1024, 0) in _seen[("edges_chains", "A", 3)]
    assert list(_seen[("hbm_at_64_threads", "A", 3)]) == [(GENERAL, 3, 64, 0)]
    for group in ("drained", "drained_sources"):
        for npw in (1, 2, 3):
            assert all(key[0] == RING for key in _seen[(group, "A", npw)]), (group, npw)
