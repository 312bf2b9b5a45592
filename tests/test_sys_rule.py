"""CPU suite: which pairs the systolic DAG kernel popoa_sys_kernel<NPW, BLOCK> takes and with what ring depth, near limit, saved columns and LDS (choose_sys and
search_saved_columns of the packer, centrolign_amd/csrc/cl_stitch_plan_api.cpp, seen through the host-only entry point cl_stitch_sys_choice), restated here from the
batch alone as ring_rule restates choose_ring in tests/test_gpu_general_kernels.py; and the shapes that tests/test_gpu_sys_kernel.py runs on the device, each asserted
to be in the class it was built for.

The rule, per pair at a NumPW (cw = 4 words per cell at NumPW 1, else 8).  Rows = the shorter graph (graph 1 on a tie) + the boundary row, at most 1 024 of them; columns =
the other graph.  For each candidate near limit 2, 4, 8, 32, 128, 512, 2 047 in turn: a column's predecessors (a source's boundary column 0 included) at most `limit`
columns back are served by the row's ring, the others are SAVED columns, at most 32; H = the smallest power of two >= row span + farthest near distance + 1; the footprint
is n_rows stride 4 + saved n_rows cw 4 + n_cols 8 + predecessors 4 + saved 4 + 16 bytes with stride = H cw + (4 if cw == 8 else 8).  The limit with the smallest
footprint wins (the first of equals), and the search ends at the first limit that needs no saved column.  Taken if that footprint is at most 159 KB, no column has more than 63
predecessors and the column graph's lists hold fewer than 2^17 entries.

The column record of the kernel holds a near distance in 11 bits (hence 2 047), a slot in 5 bits (32 saved columns), an in-degree in 6 bits (63) and a list start in 17
bits: the shapes below sit at each of these limits but the last, which no pair of at most 159 KB reaches (2^17 list entries are 512 KB of LDS; asserted below)."""
import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests import helpers as H
from tests.test_gpu_general_kernels import leading_gap_batch, two_gaps_batch

LIMITS = (2, 4, 8, 32, 128, 512, 2047)
SYS_LDS_BYTES = 159 * 1024                                              # kSysLdsBytes
LDS_CLASSES = (12 * 1024, 32 * 1024, 64 * 1024, 100 * 1024, SYS_LDS_BYTES)   # read_group_switches
LDS_SPLIT = 64 * 1024
SYS = "popoa_sys_kernel"


# ---- the pair in rank space ------------------------------------------------------------------------------------------------------------------------------
def rank_space(batch, k, order="auto"):
    """per side: n, the edges as (head, tail) ranks (1-based, as the device numbers them), the sources' ranks, the in-degrees by rank, whether the side is a chain
    from its one source (the first rank) to its one sink (the last).  None: a side is empty (a pure deletion, no device launch)"""
    out = []
    for s in (0, 1):
        side = batch.side[s]
        b0, b1 = int(side.node_off[k]), int(side.node_off[k + 1])
        n = b1 - b0
        if not n:
            return None
        rank = np.empty(n, np.int64)
        rank[capi.stitch_rank_order(batch, k, s, order)[0].astype(np.int64)] = np.arange(n)
        off = side.prev_off[b0:b1 + 1].astype(np.int64)
        head = rank[np.repeat(np.arange(n), np.diff(off))] + 1
        tail = rank[side.prev_idx[int(off[0]):int(off[-1])].astype(np.int64)] + 1
        src = np.sort(rank[side.src_idx[int(side.src_off[k]):int(side.src_off[k + 1])].astype(np.int64)]) + 1
        snk = np.sort(rank[side.snk_idx[int(side.snk_off[k]):int(side.snk_off[k + 1])].astype(np.int64)]) + 1
        deg = np.bincount(head - 1, minlength=n)
        chain = (list(src) == [1] and list(snk) == [n] and deg[0] == 0 and bool(np.all(deg[1:] == 1)) and bool(np.all(head - tail == 1)))
        out.append(dict(n=n, head=head, tail=tail, src=src, deg=deg, chain=chain))
    return out


REFUSED = dict(taken=False, rows_are_graph2=False, log2_depth=0, near_limit=0, near_max=0, saved=[], lds_bytes=0)


def sys_rule(batch, k, npw, order="auto"):
    """(what cl_stitch_sys_choice must answer, what else the tests want to know about the pair); None for a pure deletion"""
    g = rank_space(batch, k, order)
    if g is None:
        return None
    s_row = 1 if g[1]["n"] < g[0]["n"] else 0
    R, Cc = g[s_row], g[1 - s_row]
    n_rows, n_cols = R["n"] + 1, Cc["n"]
    n_pred = len(R["head"]) + len(Cc["head"])
    row_span = max(int((R["head"] - R["tail"]).max()) if len(R["head"]) else 0, int(R["src"].max()))      # a source reads the boundary row
    cw = 4 if npw == 1 else 8
    dist = Cc["head"] - Cc["tail"]
    info = dict(n=(g[0]["n"], g[1]["n"]), n_rows=n_rows, n_cols=n_cols, row_span=row_span, chain_pair=g[0]["chain"] and g[1]["chain"],
                block=64 if n_rows <= 64 else 256 if n_rows <= 256 else 1024, block128=128 if 64 < n_rows <= 128 else None, tried={},
                deg_rows=R["deg"], deg_cols=Cc["deg"], src_rows=R["src"], src_cols=Cc["src"], col_dist=dist, col_tail=Cc["tail"], col_head=Cc["head"])
    if n_rows > 1024:
        return dict(REFUSED), info
    best = None
    for limit in LIMITS:
        far = set(Cc["tail"][dist > limit].tolist())
        near = dist[dist <= limit]
        nm = int(near.max()) if len(near) else 0
        if np.any(Cc["src"] > limit):
            far.add(0)
        if np.any(Cc["src"] <= limit):
            nm = max(nm, int(Cc["src"][Cc["src"] <= limit].max()))
        info["tried"][limit] = len(far)
        if len(far) > 32:
            continue
        lg = 0
        while (1 << lg) < row_span + nm + 1 and lg < 14:
            lg += 1
        stride = (1 << lg) * cw + (4 if cw == 8 else 8)
        nbytes = n_rows * stride * 4 + len(far) * n_rows * cw * 4 + n_cols * 8 + n_pred * 4 + len(far) * 4 + 16
        info["tried"][limit] = (len(far), lg, nbytes)
        if best is None or nbytes < best[0]:
            best = (nbytes, limit, nm, lg, sorted(far))
        if not far:
            break
    info["best"] = best
    taken = (best is not None and (1 << best[3]) >= row_span + best[2] + 1 and best[0] <= SYS_LDS_BYTES and int(Cc["deg"].max()) <= 63 and len(Cc["head"]) < (1 << 17))
    if not taken:
        return dict(REFUSED), info
    return dict(taken=True, rows_are_graph2=bool(s_row), log2_depth=best[3], near_limit=best[1], near_max=best[2], saved=best[4], lds_bytes=best[0]), info


def predicted_launches(batch, npw, order="auto", block128=False, force_general=False):
    """(the launches form_sys_groups makes of the pairs the rule takes, as sorted (kernel, pairs, dynamic LDS); the pairs taken).  A chain pair goes to the chain
    kernels unless CL_FORCE_GENERAL=1.  Per (workgroup size, NumPW): the LDS classes from the hungriest down, a class joining the launch open in front of it while the
    launch then still has all its workgroups resident at once (256 compute units x workgroups per unit at the launch's LDS), else opening its own"""
    members = {}
    taken = []
    for k in range(batch.n_problems):
        r = sys_rule(batch, k, int(npw[k]), order)
        if r is None or not r[0]["taken"] or (r[1]["chain_pair"] and not force_general):
            continue
        taken.append(k)
        block = r[1]["block128"] if block128 and r[1]["block128"] else r[1]["block"]
        members.setdefault((block, int(npw[k])), []).append(r[0]["lds_bytes"])
    out = []
    for (block, n), need in members.items():
        of_class = [[] for _ in LDS_CLASSES]
        for b in need:
            of_class[next((c for c in range(4) if b <= LDS_CLASSES[c]), 4)].append(b)
        have, lds = 0, 0
        for lc in range(4, -1, -1):
            if not of_class[lc]:
                continue
            if have:
                per_cu = max(1, min(160 * 1024 // max(lds, 1), 2048 // block))
                if have + len(of_class[lc]) > 256 * per_cu:
                    out.append(("%s<%d, %d>" % (SYS, n, block), have, lds))
                    have, lds = 0, 0
            have += len(of_class[lc])
            lds = max(lds, max(of_class[lc]))
        out.append(("%s<%d, %d>" % (SYS, n, block), have, lds))
    return sorted(out), taken


# ---- explicit graphs ---------------------------------------------------------------------------------------------------------------------------------------
BASE = np.random.default_rng(1000).integers(1, 5, size=12000)     # every graph mutates the same sequence, so that the alignments are not trivial


def chain(n, seed, skips=(), sources=(), orphans=(), skips_first=False, at=0):
    """nodes 0 .. n - 1 in a chain, labels BASE[at : at + n] with one in twenty changed.  skips: (tail, length) = a further edge tail -> tail + length, behind the chain's
    own edge in the head's predecessor list (in front of it with skips_first); sources: nodes that are sources as well and KEEP their chain edge; orphans: nodes j that
    lose it (j - 1 -> j + 1 instead: j is a source without predecessors, which a rank order may move).  Without orphans the chain is the only topological order: rank = id"""
    rng = np.random.default_rng(seed)
    lab = BASE[at:at + n].copy()
    mut = rng.random(n) < 0.05
    lab[mut] = rng.integers(1, 5, size=int(mut.sum()))
    own = [(i, i + 1) for i in range(n - 1) if i + 1 not in orphans]
    extra = [(t, t + d) for t, d in skips] + [(j - 1, j + 1) for j in orphans]
    assert all(0 <= u < v < n and v - u >= 2 for u, v in extra) and len(set(extra)) == len(extra), (n, extra)
    assert all(0 < j < n - 1 for j in orphans)
    # the orphans take the lowest ids: the reference's topological order (the highest free id first) then walks the chain from its own source and ranks an orphan
    # where the chain needs it, in mid-graph
    ids = {p: i for i, p in enumerate(list(orphans) + [p for p in range(n) if p not in orphans])}
    edges = [(ids[u], ids[v]) for u, v in (extra + own if skips_first else own + extra)]
    return dict(labels=[int(lab[p]) for p in sorted(ids, key=ids.get)], edges=edges, sources=sorted(ids[p] for p in {0} | set(sources) | set(orphans)), sinks=[ids[n - 1]])


def _both(pairs):
    """every pair in both orientations"""
    return H.batch_from_graphs([p for a, b in pairs for p in ((a, b), (b, a))])


# -- workgroup sizes
BLOCK_EDGES = [(63, 80), (80, 63), (64, 80), (80, 64), (127, 150), (150, 127), (128, 150), (150, 128), (255, 300), (300, 255), (256, 300), (300, 256)]
DEGENERATE = [(1, 1), (1, 2), (2, 1), (1, 300), (300, 1)]


def _sized(sizes, **kw):
    b = synth.sized_dag_batch(sizes, **kw)
    n1, n2 = b.sizes()
    assert [(int(x), int(y)) for x, y in zip(n1, n2)] == sizes
    return b


def rows_pair(rows, seed):
    """a chain of `rows` nodes against one of rows + 60 with one skip of two: the shallowest ring there is (H = 4)"""
    return chain(rows, seed), chain(rows + 60, seed + 1, skips=[(rows // 3, 2)], at=3)


def most_rows(npw):
    """the largest number of rows (nodes of the shorter graph) of a rows_pair the rule takes at that NumPW: 1 023 at NumPW 1, where 1 024 rows with the boundary row
    are 116 KB; at NumPW 2 and 3 a row of the shallowest ring is 144 bytes and the 159 KB run out first"""
    lo, hi = 64, 1023      # taken at lo; the footprint grows with the rows
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if sys_rule(H.batch_from_graphs([rows_pair(mid, 700)]), 0, npw)[0]["taken"]:
            lo = mid
        else:
            hi = mid - 1
    return lo


_most = {}


def most_rows_cached(npw):
    if npw not in _most:
        _most[npw] = most_rows(npw)
    return _most[npw]


def most_rows_batch():
    sizes = sorted({most_rows_cached(npw) + more for npw in (1, 2, 3) for more in (0, 1)})
    return _both([rows_pair(r, 700) for r in sizes]), sizes


# -- ring depth: (the near limit that is to win, the farthest near distance, nodes of the row graph, nodes of the column graph)
# H = 2^ceil(log2(1 + near + 1)) with a row graph that is a chain; more than 2 H columns, so that the ring wraps — but for 2 047 (H = 4 096, 128 KB for the boundary
# row and one node at NumPW 1, which leaves the column records of 2 600 columns) and for 1 500 (H = 2 048: 4 200 columns at NumPW 1)
RING_SHAPES = [(2, 2, 3, 60), (4, 4, 3, 60), (8, 8, 3, 80), (32, 20, 3, 140), (32, 32, 3, 200), (128, 100, 3, 400), (128, 128, 3, 600), (512, 400, 2, 1200),
               (512, 512, 2, 2200), (2047, 1500, 1, 4200), (2047, 2047, 1, 2500)]


def ring_graph(limit, near, n_cols, seed):
    """a column graph for which the rule's search ends at `limit` with near_max = `near`: 33 skips of `near` columns from 33 tails spread over the graph (too many saved
    columns for every smaller limit — none needed for the limit 2), one skip of limit + 1 and, so that the next limit would need a deeper ring and lose, one of the
    next limit (both saved).  Returns (graph, the saved columns as 1-based ranks)"""
    nxt = LIMITS[LIMITS.index(limit) + 1] if limit != 2047 else None
    fillers = [(i * ((n_cols - near - 1) // 33), near) for i in range(33)] if near > 2 else [(5, 2), (n_cols - 9, 2)]
    far = [(7, limit + 1)] + ([(11, nxt)] if nxt and 11 + nxt < n_cols else [])
    return chain(n_cols, seed, skips=fillers + far), sorted(t + 1 for t, _ in far)


def ring_depth_batch():
    pairs = []
    for i, (limit, near, rows, n_cols) in enumerate(RING_SHAPES):
        pairs.append((chain(rows, 710 + i, at=8), ring_graph(limit, near, n_cols, 730 + i)[0]))
    return _both(pairs)


# -- saved columns
def saved_graph(k, n_cols, seed, length=200, **kw):
    """k skips of `length` columns from the tails 20, 23, 26, ...: k saved columns at the limit 2"""
    return chain(n_cols, seed, skips=[(20 + 3 * i, length) for i in range(k)], **kw)


def saved_columns_batch():
    """the pairs, both orientations each (pair 2 i and 2 i + 1):
    0-3  K = 1, 2, 32 saved columns against 40 rows, and 33 (the skips 100 columns long), which the limit 2 refuses as 4, 8 and 32 do: with 30 rows the search ends at
         128 with a ring of 128 columns and nothing saved
    4    K = 33 against 200 rows: that ring is beyond 159 KB at every NumPW — another kernel takes the pair
    5    the far edge in FRONT of the chain's own in the predecessor list (f0 set, f1 clear; elsewhere f1 set, f0 clear)
    6    saved columns that are forks with two predecessors themselves, read from 2 columns on (near, by a skip), 1 (the chain) and 200 (far)
    7    a late source (with its chain edge: two predecessors, the boundary column far) — column 0 saved in slot 0, alone
    8    ... together with two other saved columns; 9: the same source without predecessors (an orphan), under the reference's rank order
    10   the second source at column 2, within the limit: nothing saved, and near_max is 2 — 11: the same graph without that source: near_max 1"""
    rows = chain(40, 750, skips=[(11, 2)], at=15)
    pairs = [(rows, saved_graph(k, 420, 751 + k)) for k in (1, 2, 32)] + [(chain(30, 759, skips=[(11, 2)], at=15), saved_graph(33, 420, 784, length=100))]
    pairs.append((chain(200, 760, skips=[(11, 2)], at=15), saved_graph(33, 420, 761, length=100)))
    pairs.append((rows, saved_graph(3, 420, 762, skips_first=True)))
    pairs.append((rows, chain(420, 763, skips=[(t, d) for t in (30, 90) for d in (2, 200)] + [(27, 3), (87, 3)])))
    pairs.append((rows, chain(420, 764, sources=[150])))
    pairs.append((rows, chain(420, 765, skips=[(40, 150), (60, 300)], sources=[150, 380])))
    pairs.append((rows, chain(420, 766, skips=[(40, 150)], orphans=[170])))
    pairs.append((rows, chain(420, 767, sources=[1])))
    pairs.append((rows, chain(420, 767)))
    return _both(pairs)


def far_fork():
    return capi.StitchBatch.concat([synth.far_fork_batch([size], seed=770 + n_far, n_far=n_far, far_min=100, far_max=600) for size, n_far in (((120, 900), 3), ((100, 700), 2), ((60, 1000), 6))])


# -- cells
def mixed_graph(n, seed, at=0, orphan=None):
    """in-degrees 1, 2 and 3, a source with one predecessor (the straight-line cell's second predecessor = the boundary) and one with two (the general cell), every
    30 nodes; an orphan as well (a source without predecessors in mid-graph).  A late source of the row graph reads the boundary row from where it is — its rank
    counts into the row span and so into H — which is why the row graphs are short"""
    skips, sources = [], []
    for a in range(6, n - 20, 30):
        skips += [(a, 2), (a + 6, 2), (a + 5, 3)]       # a + 2: in-degree 2; a + 8: in-degree 3
        sources += [a + 12, a + 18]                     # a + 12: a source with one predecessor; a + 18: with two
        skips += [(a + 16, 2)]
    return chain(n, seed, skips=skips, sources=sources, orphans=[orphan] if orphan else (), at=at)


def fan_graph(n, seed, node, deg, at=0):
    """node `node` with `deg` predecessors: the chain's and deg - 1 skips"""
    return chain(n, seed, skips=[(node - d, d) for d in range(2, deg + 1)], at=at)


def cells_batch():
    """0-1 in-degrees and sources of every kind on both sides; 2 a column with 63 predecessors (the 6-bit field full), 3 with 64 (refused); 4 a row with 64 (no limit
    on that side, but 64 distinct predecessors are a row span of 64 and a ring of 128 columns: 71 rows of it are 148 KB at NumPW 1 and too much at NumPW 2 and 3)"""
    pairs = [(mixed_graph(50, 780, orphan=30), mixed_graph(130, 781, at=4, orphan=65)), (mixed_graph(60, 782, orphan=33), mixed_graph(101, 783, at=2, orphan=65)),
             (chain(30, 784, skips=[(9, 2)]), fan_graph(120, 785, 80, 63)), (chain(30, 784, skips=[(9, 2)]), fan_graph(120, 786, 80, 64)),
             (fan_graph(70, 787, 68, 64), mixed_graph(130, 788, at=4))]
    return _both(pairs)


# -- LDS classes: (rows, a skip in the row graph: the row span that alone makes the ring deep).  Above 64 KB: 63 rows at every NumPW; 100 rows with the span 40 at
# NumPW 1 and 20 at NumPW 2, 3; 200 rows with 20 at NumPW 1 and 10 at 2, 3; 500 rows at every NumPW; 300 rows in a plain chain (H = 4): 1 024 threads with at most 64 KB
LDS_SHAPES = [(63, 40), (100, 40), (100, 20), (200, 20), (200, 10), (500, 5), (300, 0)]


SMALL_LDS_ROWS = (300, 150, 100)


def lds_batch():
    pairs = [(chain(rows, 790 + i, skips=[(4, span), (1, 2)] if span else []), chain(rows + 40, 800 + i, skips=[(rows // 3, 2)], at=5)) for i, (rows, span) in enumerate(LDS_SHAPES)]
    # 63 rows with a ring of 128 columns (the near distance 100 of ring_graph): 131 KB at NumPW 1, the 64-thread workgroup's largest
    return _both(pairs + [(chain(63, 798, skips=[(1, 2)]), ring_graph(128, 100, 400, 799)[0])])


GROUPS = {
    "edges_dags": lambda: _sized(BLOCK_EDGES, seed=702),
    "edges_dense_dags": lambda: _sized(BLOCK_EDGES, seed=703, extra_edge_p=0.4, skip_max=6, alphabet=2),
    "degenerate": lambda: capi.StitchBatch.concat([synth.linear_batch(DEGENERATE, seed=704), _sized(DEGENERATE, seed=705),
                                                   _sized(DEGENERATE, seed=706, extra_edge_p=0.4, skip_max=6, alphabet=2)]),
    "most_rows": lambda: most_rows_batch()[0],
    "random_dags": lambda: synth.random_dag_batch(200, seed=707, max_n=60),
    "ring_depth": ring_depth_batch,
    "saved_columns": saved_columns_batch,
    "far_fork": far_fork,
    "cells": cells_batch,
    "lds_classes": lds_batch,
    # ... and at most 64 KB in every launch: 1 024, 256 and 256 (128) threads with rings of four columns
    "small_lds": lambda: _both([rows_pair(rows, 810 + rows) for rows in SMALL_LDS_ROWS]),
    "leading_gap_through_a_bubble": leading_gap_batch,
    "two_gaps_at_a_source": two_gaps_batch,
}
# groups that also run under CL_RANK_ORDER=lifo: the packer's own order ranks a source without predecessors first; in the reference's order it sits in mid-graph, next
# to the node it feeds (see RANK_ORDER in tests/test_gpu_general_kernels.py)
LIFO_TOO = ("cells", "saved_columns", "two_gaps_at_a_source")
# CL_FORCE_GENERAL=1: the chain pairs among them (1 x 1 is always one) go past the chain kernels, to choose_sys
FORCE_GENERAL = ("degenerate",)
_batches = {}


def batch_of(group):
    if group not in _batches:
        _batches[group] = GROUPS[group]()
    return _batches[group]


def runs():
    """(group, rank order) of every plan the device tests make"""
    return [(g, o) for g in sorted(GROUPS) for o in (("auto", "lifo") if g in LIFO_TOO else ("auto",))]


# ---- the restatement is the packer's -----------------------------------------------------------------------------------------------------------------------
def _same(batch, order="auto", npws=(1, 2, 3)):
    for k in range(batch.n_problems):
        for npw in npws:
            want = sys_rule(batch, k, npw, order)
            got = capi.stitch_sys_choice(batch, k, npw, order)
            assert got == (want[0] if want else REFUSED), (k, npw, order, got, want and want[0], want and want[1]["tried"])


@pytest.mark.parametrize("group,order", runs())
def test_the_rule_is_the_packers_on_the_crafted_batches(group, order):
    _same(batch_of(group), order)


def test_the_rule_is_the_packers_on_random_pairs():
    for order in ("auto", "lifo", "level"):
        _same(synth.random_dag_batch(150, seed=720, max_n=90, skip_max=9), order)
    _same(synth.random_dag_batch(60, seed=721, max_n=300, extra_edge_p=0.5, skip_max=40, allow_empty=False))
    _same(_sized([(int(a), int(b)) for a, b in np.random.default_rng(722).integers(1, 700, size=(60, 2))], seed=723, skip_max=12))
    _same(_sized([(1023, 1030), (1030, 1023), (1024, 1030), (1030, 1024), (1025, 1200), (900, 20000)], seed=724), npws=(1, 3))
    _same(synth.far_fork_batch([(int(a), int(b)) for a, b in np.random.default_rng(725).integers([20, 400], [400, 3000], size=(40, 2))], seed=726, n_far=5, far_min=50, far_max=2500))
    _same(synth.far_fork_batch([(3, 5000), (1, 4000), (2, 9000), (8, 6000)] * 5, seed=727, n_far=40, far_min=600, far_max=2300))


def test_the_entry_point_refuses_bad_arguments():
    b = synth.random_dag_batch(3, seed=1, allow_empty=False)
    for k, npw in ((3, 1), (0, 0), (0, 4)):
        with pytest.raises(capi.ClError):
            capi.stitch_sys_choice(b, k, npw)
    empty = synth.linear_batch([(40, 0), (0, 3)], seed=2)
    assert capi.stitch_sys_choice(empty, 0, 1) == REFUSED and capi.stitch_sys_choice(empty, 1, 2) == REFUSED


# ---- the shapes are what they are for ----------------------------------------------------------------------------------------------------------------------
def _rule(group, k, npw, order="auto"):
    return sys_rule(batch_of(group), k, npw, order)


def test_workgroup_sizes_and_the_most_rows():
    for group in ("edges_dags", "edges_dense_dags"):
        for k, (n1, n2) in enumerate(BLOCK_EDGES):
            for npw in (1, 2, 3):
                c, x = _rule(group, k, npw)
                rows = min(n1, n2) + 1
                assert c["taken"] and not x["chain_pair"] and c["rows_are_graph2"] == (n2 < n1), (group, k, npw)
                assert x["block"] == (64 if rows <= 64 else 256 if rows <= 256 else 1024) and x["block128"] == (128 if 64 < rows <= 128 else None)
    assert {min(s) + 1 for s in BLOCK_EDGES} == {64, 65, 128, 129, 256, 257}
    # the most rows: 1 023 nodes at NumPW 1 (the 1 024 threads), fewer at NumPW 2 and 3 (H >= 4 always: 144 bytes a row), and one more is refused
    most = {npw: most_rows_cached(npw) for npw in (1, 2, 3)}
    assert most[1] == 1023 and most[2] == most[3] and 900 < most[2] < 1023, most
    b, sizes = most_rows_batch()
    assert sizes == sorted({most[1], most[1] + 1, most[2], most[2] + 1})
    for i, rows in enumerate(sizes):
        for k in (2 * i, 2 * i + 1):
            for npw in (1, 2, 3):
                c, x = sys_rule(b, k, npw)
                assert c["taken"] == (rows <= most[npw]) and not x["chain_pair"], (rows, k, npw, c)
                assert not c["taken"] or (c["log2_depth"] == 2 and x["block"] == 1024 and c["lds_bytes"] > LDS_SPLIT), (rows, npw, c)
    # pairs of one node: all of them taken, rings of 4 to 16 columns (under CL_FORCE_GENERAL=1, which the chain pairs among them need)
    d = batch_of("degenerate")
    assert d.n_problems == 3 * len(DEGENERATE)
    for k in range(d.n_problems):
        for npw in (1, 2, 3):
            c, x = sys_rule(d, k, npw)
            assert c["taken"] and c["log2_depth"] <= 4 and not c["saved"] and x["block"] == 64 and x["n_rows"] <= 3, (k, npw, c)
    assert sum(sys_rule(d, k, 1)[1]["chain_pair"] for k in range(d.n_problems)) >= len(DEGENERATE)


def test_ring_depths():
    b = batch_of("ring_depth")
    logs = {1: set(), 2: set(), 3: set()}
    for i, (limit, near, rows, n_cols) in enumerate(RING_SHAPES):
        saved = ring_graph(limit, near, n_cols, 730 + i)[1]
        depth = 1 << int(np.ceil(np.log2(1 + near + 1)))
        for k in (2 * i, 2 * i + 1):
            for npw in (1, 2, 3):
                c, x = sys_rule(b, k, npw)
                fits = (rows + 1) * (depth * (4 if npw == 1 else 8) + 4) * 4 + 12 * n_cols <= SYS_LDS_BYTES
                if not fits:      # 2 047 and 1 500 at NumPW 2 and 3: no smaller limit has few enough saved columns, so another kernel takes the pair
                    assert not c["taken"] and near >= 1500 and npw > 1, (limit, near, npw, c, x["tried"])
                    continue
                assert c["taken"] and c["rows_are_graph2"] == bool(k % 2) and not x["chain_pair"], (limit, near, npw, c, x["tried"])
                assert (c["near_limit"], c["near_max"], 1 << c["log2_depth"], c["saved"]) == (limit, near, depth, saved), (limit, near, npw, c, x["tried"])
                # a read at exactly near_max and one at limit + 1; every smaller limit was refused for its saved columns, but for 2
                assert near in x["col_dist"] and limit + 1 in x["col_dist"] and all(x["tried"][s] in (33, 34, 35) for s in LIMITS if s < limit and near > 2)
                assert n_cols > 2 * depth or (near >= 1500 and (rows + 1) * (depth * 4 + 8) * 4 + 12 * (2 * depth) > SYS_LDS_BYTES), (limit, near)
                logs[npw].add(c["log2_depth"])
    # every depth the rule can give a pair: 2 (H >= 4: a row span and a near distance of 1 at the least) up to the deepest that fits the boundary row and one node,
    # 159 KB >= 2 rows x (H cw + pad) x 4: H = 4 096 at NumPW 1 (which takes the near distance 2 047, the 11-bit field full), 2 048 at NumPW 2 and 3
    assert logs[1] == set(range(2, 13)), logs
    for npw in (2, 3):
        lds = lambda lg: 2 * ((1 << lg) * 8 + 4) * 4
        assert lds(11) <= SYS_LDS_BYTES < lds(12) and logs[npw] == set(range(2, 11)), logs
    # (log 11 at NumPW 2 and 3 needs a near distance above 1 022 on one row node, and 128 KB of ring leave 159 - 128 KB for at most 2 600 columns of records and lists)
    c, x = _rule("ring_depth", 2 * 9, 2)
    assert not c["taken"] and x["best"][3] == 11 and x["best"][0] > SYS_LDS_BYTES, x["best"]


def test_saved_columns():
    b = batch_of("saved_columns")
    tails = lambda k: [21 + 3 * i for i in range(k)]      # ranks are 1-based
    for i, k in enumerate((1, 2, 32)):
        for npw in (1, 2, 3):
            for kk in (2 * i, 2 * i + 1):
                c, x = sys_rule(b, kk, npw)
                assert c["taken"] and c["near_limit"] == 2 and c["log2_depth"] == 2 and c["saved"] == tails(k) and c["rows_are_graph2"] == bool(kk % 2), (k, npw, c)
    for npw in (1, 2, 3):
        c, x = sys_rule(b, 6, npw)       # K = 33: refused at 2 .. 32, the search moves on to 128: no saved column, a ring of 128 columns
        assert [x["tried"][s] for s in (2, 4, 8, 32)] == [33] * 4 and c["taken"] and (c["near_limit"], c["near_max"], c["log2_depth"], c["saved"]) == (128, 100, 7, []), (npw, c)
        c, x = sys_rule(b, 8, npw)       # ... which 200 rows cannot have: not a systolic pair
        assert [x["tried"][s] for s in (2, 4, 8, 32)] == [33] * 4 and not c["taken"] and x["best"][1] == 128 and x["best"][0] > SYS_LDS_BYTES, (npw, c, x["best"])
        c, x = sys_rule(b, 10, npw)      # the far predecessor first in the list
        head = int(np.flatnonzero(x["col_dist"] == 200)[0])
        assert c["taken"] and c["saved"] == tails(3) and x["col_dist"][head + 1] == 1 and x["col_head"][head + 1] == x["col_head"][head], (npw, c)
        c, x = sys_rule(b, 0, npw)       # ... and last
        head = int(np.flatnonzero(x["col_dist"] == 200)[0])
        assert x["col_dist"][head - 1] == 1 and x["col_head"][head - 1] == x["col_head"][head]
        c, x = sys_rule(b, 12, npw)      # saved forks: two predecessors each, read from 1, 2 and 200 columns on
        assert c["taken"] and c["near_limit"] == 4 and c["saved"] == [31, 91], (npw, c, x["tried"])
        for col in c["saved"]:
            assert x["deg_cols"][col - 1] == 2 and {1, 2, 200} <= set(x["col_dist"][x["col_tail"] == col].tolist()), (npw, col)
        c, x = sys_rule(b, 14, npw)      # a late source: the boundary column, alone
        assert c["taken"] and c["saved"] == [0] and c["near_max"] == 1 and list(x["src_cols"]) == [1, 151] and x["deg_cols"][150] == 1, (npw, c)
        c, x = sys_rule(b, 16, npw)      # ... and with others
        assert c["taken"] and c["saved"] == [0, 41, 61] and list(x["src_cols"]) == [1, 151, 381], (npw, c)
        c, x = sys_rule(b, 18, npw, "lifo")      # ... and without predecessors, where the reference's order leaves it in mid-graph
        assert c["taken"] and c["saved"] == [0, 41] and len(x["src_cols"]) == 2 and x["src_cols"][1] > 100 and x["deg_cols"][x["src_cols"][1] - 1] == 0, (npw, c, x["src_cols"])
        c, x = sys_rule(b, 20, npw)      # the source within the limit: nothing saved, and the ring serves the boundary column two columns back
        assert c["taken"] and c["saved"] == [] and (c["near_limit"], c["near_max"]) == (2, 2) and list(x["src_cols"]) == [1, 2] and x["col_dist"].max() == 1, (npw, c)
        c, x = sys_rule(b, 22, npw)      # ... which without that source reads one column back at the most
        assert c["taken"] and c["saved"] == [] and (c["near_limit"], c["near_max"], c["log2_depth"]) == (2, 1, 2) and list(x["src_cols"]) == [1], (npw, c)
    f = batch_of("far_fork")
    counts = set()
    for k in range(f.n_problems):
        for npw in (1, 2, 3):
            c, x = sys_rule(f, k, npw)
            assert c["taken"] and c["saved"] and x["col_dist"].max() >= 100, (k, npw, c)
            counts.add(len(c["saved"]))
    assert len(counts) >= 2, counts


def _cell_kinds(x):
    """(fastR, fastC) combinations a pair's cells fall into: a row / column takes the straight-line cell with one or two predecessors, a source's boundary counted"""
    out = []
    for deg, src in ((x["deg_rows"], x["src_rows"]), (x["deg_cols"], x["src_cols"])):
        nq = deg.copy()
        nq[src - 1] += 1
        out.append({bool(v) for v in ((nq >= 1) & (nq <= 2))})
    return {(r, c) for r in out[0] for c in out[1]}, out


def test_cells():
    b = batch_of("cells")
    for npw in (1, 2, 3):
        for k in range(4):
            for order in ("auto", "lifo"):
                c, x = sys_rule(b, k, npw, order)
                kinds, _ = _cell_kinds(x)
                assert c["taken"] and kinds == {(False, False), (False, True), (True, False), (True, True)}, (k, npw, order, kinds)
                for deg, src in ((x["deg_rows"], x["src_rows"]), (x["deg_cols"], x["src_cols"])):
                    nq = deg.copy()
                    nq[src - 1] += 1
                    is_src = np.zeros(len(deg), bool)
                    is_src[src - 1] = True
                    # in-degree 1, 2, 3; a source with one predecessor and with two; a second source in mid-graph
                    assert {1, 2, 3} <= set(deg[~is_src].tolist()) and {1, 2} <= set(deg[is_src].tolist()) and src.max() > 20, (k, npw, order)
        c, x = sys_rule(b, 2, npw, "lifo")
        assert any(d == 0 for d in x["deg_cols"][x["src_cols"][1:] - 1]) and x["src_cols"][x["deg_cols"][x["src_cols"] - 1] == 0].max() > 20      # the orphan stays in mid-graph
        c, x = sys_rule(b, 4, npw)
        assert c["taken"] and x["deg_cols"].max() == 63, (npw, c)
        c, x = sys_rule(b, 6, npw)
        assert not c["taken"] and x["deg_cols"].max() == 64 and x["best"][0] <= SYS_LDS_BYTES, (npw, c)
        c, x = sys_rule(b, 8, npw)
        assert c["taken"] == (npw == 1) and x["deg_rows"].max() == 64 and x["row_span"] == 64 and x["best"][3] == 7 and (npw == 1 or x["best"][0] > SYS_LDS_BYTES), (npw, c)
    for group in ("leading_gap_through_a_bubble", "two_gaps_at_a_source"):
        g = batch_of(group)
        for k in range(g.n_problems):
            c, x = sys_rule(g, k, 1)
            assert c["taken"] or x["chain_pair"], (group, k)
        assert sum(not sys_rule(g, k, 1)[1]["chain_pair"] for k in range(g.n_problems)) >= g.n_problems // 2, group


def test_lds_classes_and_list_lengths():
    b = batch_of("lds_classes")
    seen = set()
    for group in ("lds_classes", "edges_dags", "most_rows", "small_lds"):
        g = batch_of(group)
        for k in range(g.n_problems):
            for npw in (1, 2, 3):
                c, x = sys_rule(g, k, npw)
                if c["taken"]:
                    seen |= {(npw, blk, c["lds_bytes"] > LDS_SPLIT) for blk in (x["block"], x["block128"]) if blk}
    # both LDS classes for every NumPW and workgroup size — 64 threads above 64 KB: 63 rows with H = 64 (H = 128 at NumPW 1 is 131 KB)
    assert seen == {(npw, blk, big) for npw in (1, 2, 3) for blk in (64, 128, 256, 1024) for big in (False, True)}, sorted(seen)
    c, _ = sys_rule(b, 2 * len(LDS_SHAPES), 1)
    assert c["log2_depth"] == 7 and 64 * (128 * 4 + 8) * 4 == 133120 < c["lds_bytes"] < 140 * 1024, c
    # the 17-bit list start: a column list of 2^17 entries is 512 KB of LDS, so the footprint refuses long before the field is full
    assert (1 << 17) * 4 > SYS_LDS_BYTES


def test_the_classes_of_a_mixed_batch_share_a_launch():
    b = capi.StitchBatch.concat([batch_of("lds_classes"), batch_of("edges_dags")])
    for npw in (1, 2, 3):
        launches, taken = predicted_launches(b, np.full(b.n_problems, npw, np.uint8))
        classes = {}
        for k in taken:
            c, x = sys_rule(b, k, npw)
            classes.setdefault(x["block"], set()).add(next((i for i in range(4) if c["lds_bytes"] <= LDS_CLASSES[i]), 4))
        assert len(launches) == len(classes) == 3 and all(len(v) >= 2 for v in classes.values()), (npw, launches, classes)
