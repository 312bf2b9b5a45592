"""CPU suite: the topological order the device ranks a subgraph's nodes by (cl_stitch_rank_order = choose_rank_order of the packer, centrolign_amd/csrc/cl_stitch_plan_api.cpp; round 5).
The result of a subproblem does not depend on the order (that is what the -m gpu parity tests hold: reference order = level order = the choice); what is checked here is
the host logic: every order returned is a topological order; chains and graphs whose bubbles have one short branch keep the reference's order
(topological_order.hpp:12-60, restated in oracle/); a bubble with two long branches is interleaved by the level order, which the choice then takes; the counts
describe the order returned."""
import numpy as np

from centrolign_amd import capi, synth


def preds_of(batch, k, side):
    s = batch.side[side]
    lo, hi = int(s.node_off[k]), int(s.node_off[k + 1])
    out = []
    for v in range(lo, hi):
        out.append([int(x) for x in s.prev_idx[int(s.prev_off[v]):int(s.prev_off[v + 1])]])
    return out


def reads(order, preds, sources):
    rank = np.zeros(len(order), np.int64)
    rank[order] = np.arange(len(order))
    back = [int(rank[v] - rank[p]) for v in range(len(order)) for p in preds[v]] + [int(rank[s]) + 1 for s in sources]
    return sum(b > 4 for b in back), max(back)


def sources_of(batch, k, side):
    s = batch.side[side]
    return [int(x) for x in s.src_idx[int(s.src_off[k]):int(s.src_off[k + 1])]]


def kahn_lifo(preds):
    """topological_order.hpp:12-60 restated: Kahn with a LIFO stack seeded with the sources in ascending id order; a node's successors are visited in the order the
    next lists hold them (here: derived from the previous lists, ascending successor id per predecessor)"""
    n = len(preds)
    nxt = [[] for _ in range(n)]
    indeg = [len(p) for p in preds]
    for v in range(n):
        for p in preds[v]:
            nxt[p].append(v)
    stack = [v for v in range(n) if indeg[v] == 0]
    order = []
    while stack:
        v = stack.pop()
        order.append(v)
        for w in nxt[v]:
            indeg[w] -= 1
            if indeg[w] == 0:
                stack.append(w)
    return order


def check_topological(order, preds):
    rank = np.full(len(order), -1, np.int64)
    rank[order] = np.arange(len(order))
    assert sorted(order.tolist()) == list(range(len(order)))
    assert all(rank[p] < rank[v] for v in range(len(order)) for p in preds[v])


def test_every_order_is_topological_and_the_counts_are_its_own():
    b = synth.random_dag_batch(120, seed=3, max_n=50)
    b2 = synth.near_chain_batch([(300, 280), (90, 700), (500, 40)], seed=5, n_long=(2, 2), long_min=30, long_max=80, long_other=6)
    for batch in (b, b2):
        for k in range(batch.n_problems):
            for side in (0, 1):
                preds, srcs = preds_of(batch, k, side), sources_of(batch, k, side)
                if not preds:
                    continue
                got = {}
                for mode in ("lifo", "level", "auto"):
                    order, far, longest = capi.stitch_rank_order(batch, k, side, mode)
                    check_topological(order, preds)
                    assert (far, longest) == reads(order, preds, srcs), (k, side, mode)
                    got[mode] = (order.tolist(), far, longest)
                # the choice is one of the two, and never reads further than the reference's order
                assert got["auto"][0] in (got["lifo"][0], got["level"][0])
                assert got["auto"][1:] <= got["lifo"][1:]
                if got["level"][1:] >= got["lifo"][1:]:
                    assert got["auto"][0] == got["lifo"][0]      # ties keep the reference's order


def test_the_reference_order_is_the_oracles_and_chains_keep_it():
    b = synth.random_dag_batch(60, seed=9, max_n=40)
    for k in range(b.n_problems):
        for side in (0, 1):
            n = int(b.side[side].node_off[k + 1] - b.side[side].node_off[k])
            if n == 0:
                continue
            order, _, _ = capi.stitch_rank_order(b, k, side, "lifo")
            assert order.tolist() == kahn_lifo(preds_of(b, k, side))
    lin = synth.linear_batch([(40, 50), (7, 900), (1, 1), (300, 3)], seed=2)
    for k in range(lin.n_problems):
        for side in (0, 1):
            a, far, longest = capi.stitch_rank_order(lin, k, side, "auto")
            l, _, _ = capi.stitch_rank_order(lin, k, side, "level")
            assert a.tolist() == l.tolist() and far == 0 and longest == 1


def test_two_long_branches_are_interleaved_and_one_short_branch_changes_nothing():
    # two-long-branch bubbles: the reference's order reads a whole branch back, the level order a few ranks
    b = synth.near_chain_batch([(3000, 3200), (700, 650)], seed=41, p_snp=0.03, p_del=0.01, n_long=(2, 2), long_min=100, long_max=300, long_other=12)
    for k in range(b.n_problems):
        for side in (0, 1):
            _, far_ref, longest_ref = capi.stitch_rank_order(b, k, side, "lifo")
            order, far, longest = capi.stitch_rank_order(b, k, side, "auto")
            lvl, far_l, longest_l = capi.stitch_rank_order(b, k, side, "level")
            assert longest_ref >= 100 and longest <= 32 and far < far_ref, (k, side, far_ref, longest_ref, far, longest)
            assert order.tolist() == lvl.tolist()
    # one long and one short branch (a whole-unit indel): one far read per bubble in ANY order — the reference's order stays
    b = synth.near_chain_batch([(900, 1000), (400, 2000)], seed=5, n_long=(1, 2), long_min=150, long_max=300)
    for k in range(b.n_problems):
        for side in (0, 1):
            ref, far_ref, _ = capi.stitch_rank_order(b, k, side, "lifo")
            order, far, _ = capi.stitch_rank_order(b, k, side, "auto")
            assert far <= far_ref
            if far == far_ref:
                assert order.tolist() == ref.tolist() or capi.stitch_rank_order(b, k, side, "auto")[2] < capi.stitch_rank_order(b, k, side, "lifo")[2]
