"""popoa_lane_kernel's row-general cell (popoa_lane.h): a step that is not the usual one takes the general cell, or — in the shape with row predecessors up to two
rows back, in a strip that runs both conveyor stages, in a chunk whose columns are all plain chain columns — the row-general cell.  That cell drops only terms that are
-inf there, so the result must be the oracle's AND, byte for byte, what CL_LANE_CELLS=general (every such step on the general cell) gives.  The cases put row and column
features on both sides of every boundary that decides between the two cells: bubble rows with and without bubble columns in the same chunk, strips of chain rows,
sources, saved columns, the shape with row predecessors up to four back (the general cell alone).

The graphs are built explicitly, so that every feature sits at a known rank: what matters to the kernel is strips of 64 rows, chunks of 32 steps, a lag of three chunks
between neighbouring strips and a hand-off window of 128 columns — pairs of at most 140 rows x about 200 columns show all of it.  (Rows are the SHORTER graph of a pair.
The pairs with a second round of strips therefore have more columns than rows: 200 rows x 260 columns, the only row bubble in rows 194-196 — the second round's strip
under CL_LANE_WAVES=3 — and 270 rows x 280 columns with it in rows 260-262, the second round under 3 and 4 waves; a 200 x 150 pair rides along, its rows the 150.)"""
import numpy as np
import pytest

from centrolign_amd import capi, synth
from oracle import pyoracle as po
from tests import helpers as H

pytestmark = pytest.mark.gpu

ALPHABET = b"ACGT"


def _graph(n, seed, snps=(), dels=(), srcs=(), multi=()):
    """a chain of n positions.  snps: positions with a second node (an SNP bubble); multi: {position: alleles} (in-degree = alleles behind it); dels: (p, length)
    = an edge from position p - 1 over `length` positions; srcs: positions with a second node that is a SOURCE (no edge into it).  Node ids follow the positions, the
    nodes of one position next to one another (the second sources first).  Returns (graph, ids: position -> node ids)"""
    rng = np.random.default_rng(seed)
    base = np.random.default_rng(1000).integers(0, 4, size=4096)     # every graph mutates the same sequence, so that the alignments are not trivial
    alleles = {p: 2 for p in snps}
    alleles.update(multi)
    srcs = sorted(srcs)
    labels = [ALPHABET[int(rng.integers(0, 4))] for _ in srcs]       # the second sources take the lowest ids: the device's topological order (highest free id first)
    sources, ids = list(range(len(srcs))), []                        # then walks the chain from its own source and ranks a second source where the chain needs it
    for p in range(n):
        k = alleles.get(p, 1)
        ids.append(list(range(len(labels), len(labels) + k)) + ([srcs.index(p)] if p in srcs else []))
        for a in range(k):
            lab = int(base[p]) if a == 0 and rng.random() > 0.05 else int(rng.integers(0, 4))
            labels.append(ALPHABET[(lab + a) % 4])
    edges = []
    for p in range(1, n):
        for u in ids[p - 1]:
            for v in ids[p]:
                if v not in sources:
                    edges.append((u, v))
    for p, length in dels:
        edges.append((ids[p - 1][0], ids[p + length][0]))
    g = dict(labels=labels, edges=edges, sources=sources + [ids[0][0]], sinks=[ids[n - 1][0]])
    assert len(ids[0]) == 1 and len(ids[n - 1]) == 1
    return g, ids


@pytest.fixture(autouse=True)
def _reference_rank_order(monkeypatch):
    """the reference's topological order (every bubble here is a single node: the packer's own choice is the same order, except that it ranks a second source first,
    which takes the pair away from this kernel — in the reference's order the source sits in the middle, next to the node it feeds)"""
    monkeypatch.setenv("CL_RANK_ORDER", "lifo")


def _ranks(batch, k, side, nodes):
    order = capi.stitch_rank_order(batch, k, side, "lifo")[0]
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return sorted(int(rank[v]) + 1 for v in nodes)       # 1-based, as the kernel's rows and columns


class Case:
    def __init__(self, name, rows, cols, where=()):
        """rows / cols: arguments of _graph for the row graph (the shorter one) and the column graph; where: (side 'r' / 'c', positions, lowest rank, highest rank)
        the ranks the nodes of those positions must have"""
        self.name, self.rows, self.cols, self.where = name, rows, cols, where


R, C = 140, 200    # three strips (the last of 12 rows), seven chunks of columns


def _cases_rows():
    out = []
    for name, p in (("strip0", 20), ("strip1", 90), ("last_partial_strip", 133)):
        out.append(Case("row_bubble_" + name, dict(n=R, seed=1, snps=[p], dels=[(p + 3, 1)]), dict(n=C, seed=2), [("r", [p], p + 1, p + 2)]))
    # rows 63-66: row 65's predecessor two back comes over the hand-off
    out.append(Case("row_bubble_across_strips", dict(n=R - 1, seed=3, snps=[63]), dict(n=C, seed=4), [("r", [62, 63, 64], 63, 66)]))
    out.append(Case("row_deletion_across_strips", dict(n=R, seed=5, dels=[(64, 1)]), dict(n=C, seed=6), [("r", [63, 65], 64, 66)]))
    return out


def _cases_cols():
    out = []
    for name, p in (("first", 1), ("chunk_edge", 31), ("strip_width", 63), ("window_wrap", 127), ("last", C - 3)):
        out.append(Case("col_snp_" + name, dict(n=R, seed=7), dict(n=C - 1, seed=8 + p, snps=[p]), [("c", [p], p + 1, p + 2)]))
        out.append(Case("col_deletion_" + name, dict(n=R, seed=9), dict(n=C, seed=10 + p, dels=[(p, 1)]), [("c", [p + 1], p + 2, p + 2)]))
    return out


def _cases_both():
    return [
        # a row bubble and a column bubble that meet in different lanes of one step, and in one cell (bubble row x bubble column: lane 19 at step 19 + 39)
        Case("row_and_col_bubbles", dict(n=R, seed=11, snps=[20, 100], dels=[(70, 1)]), dict(n=C, seed=12, snps=[40, 150], dels=[(90, 1), (120, 2)])),
        Case("bubbles_everywhere", dict(n=R, seed=13, snps=list(range(5, R - 5, 17))), dict(n=C, seed=14, snps=list(range(3, C - 5, 23)), dels=[(60, 1), (61, 2)])),
    ]


def _cases_sources():
    return [
        Case("source_in_row_strip1", dict(n=R, seed=15, srcs=[90]), dict(n=C, seed=16), [("r", [90], 91, 92)]),
        Case("source_in_columns", dict(n=R, seed=17), dict(n=C, seed=18, srcs=[100]), [("c", [100], 101, 102)]),
        Case("source_in_both", dict(n=R, seed=19, srcs=[70]), dict(n=C, seed=20, srcs=[110])),
        Case("source_row_and_col_bubbles", dict(n=R, seed=21, srcs=[30], snps=[100]), dict(n=C, seed=22, srcs=[50], snps=[51, 140])),
    ]


def _cases_distances():
    return [
        Case("col_distance_3", dict(n=R, seed=23), dict(n=C, seed=24, dels=[(50, 2), (126, 2)])),
        Case("row_distance_3_4", dict(n=R, seed=25, dels=[(30, 2), (62, 3), (100, 3)]), dict(n=C, seed=26)),           # the DR = 4 shape
        Case("row_distance_4_col_bubbles", dict(n=R, seed=27, dels=[(62, 3)]), dict(n=C, seed=28, snps=[33], dels=[(128, 2)])),
        Case("in_degree_3_rows", dict(n=R, seed=29, multi={66: 3}), dict(n=C, seed=30)),
        Case("in_degree_3_cols", dict(n=R, seed=31), dict(n=C, seed=32, multi={64: 3}, dels=[(140, 1), (140, 2)])),
    ]


def _cases_saved_columns():
    return [
        # a long bubble in the column graph (its fork is a saved column, read from 9 columns away), over chain rows ...
        Case("long_col_bubble_chain_rows", dict(n=R, seed=33), dict(n=C, seed=34, dels=[(80, 8)])),
        # ... and over strips with a row bubble: the far read lands in a step whose other lanes are plain
        Case("long_col_bubble_row_bubble", dict(n=R, seed=35, snps=[10, 80]), dict(n=C, seed=36, dels=[(120, 6)])),
        Case("two_long_col_bubbles", dict(n=R, seed=37, dels=[(100, 1)]), dict(n=C, seed=38, dels=[(30, 5), (150, 12)], snps=[90])),
    ]


def _cases_rounds():
    return [
        Case("second_round_w3", dict(n=200, seed=39, snps=[194]), dict(n=260, seed=40), [("r", [194], 195, 196)]),
        Case("second_round_w3_w4", dict(n=270, seed=41, snps=[260]), dict(n=280, seed=42), [("r", [260], 261, 262)]),
        Case("rows_150_of_200_x_150", dict(n=150, seed=43, snps=[130]), dict(n=200, seed=44)),
    ]


def _batch(cases, swap=False):
    pairs = []
    for c in cases:
        gr, gc = _graph(**c.rows)[0], _graph(**c.cols)[0]
        assert len(gr["labels"]) < len(gc["labels"]), c.name      # rows = the shorter graph
        pairs.append((gc, gr) if swap else (gr, gc))
    b = H.batch_from_graphs(pairs)
    for k, c in enumerate(cases):   # the features are where the case wants them in the DEVICE's rank order
        for side, positions, lo, hi in c.where:
            ids = _graph(**(c.rows if side == "r" else c.cols))[1]
            got = _ranks(b, k, (side == "c") != swap, [v for p in positions for v in ids[p]])
            assert lo <= got[0] and got[-1] <= hi, (c.name, side, got, lo, hi)
    return b


_oracle = {}


def _want(key, batch, **kw):
    if key not in _oracle:
        _oracle[key] = po.oracle_stitch_batch(batch, **kw)
    return _oracle[key]


def _same_bytes(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("aln_off", "pairs", "score", "route", "num_pw"))


def _check(gpu_ctx, monkeypatch, batch, want, kernel="popoa_lane_kernel", **plan_kw):
    """the plan's result is the oracle's, a second pass over the resident plan too, the wanted kernel ran, and CL_LANE_CELLS=general gives the same bytes"""
    got = {}
    for cells in ("", "general"):
        if cells:
            monkeypatch.setenv("CL_LANE_CELLS", cells)
        else:
            monkeypatch.delenv("CL_LANE_CELLS", raising=False)
        plan = gpu_ctx.plan(batch, **plan_kw)
        plan.execute(); plan.sync()
        names = [li["kernel"] for li in plan.launches() if li["n_problems"]]
        assert any(n.startswith(kernel) for n in names), (cells, names)
        got[cells] = plan.collect()
        assert got[cells].same_as(want) is None, cells
        plan.execute(); plan.sync()
        assert _same_bytes(plan.collect(), got[cells]), cells
        plan.destroy()
    monkeypatch.delenv("CL_LANE_CELLS", raising=False)
    assert _same_bytes(got[""], got["general"])


GROUPS = dict(rows=_cases_rows, cols=_cases_cols, both=_cases_both, sources=_cases_sources, distances=_cases_distances, saved_columns=_cases_saved_columns)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tiered_cell_features_at_known_places(gpu_ctx, monkeypatch, group):
    monkeypatch.setenv("CL_LANE_MIN_SWEEP", "0")
    b = _batch(GROUPS[group]())
    _check(gpu_ctx, monkeypatch, b, _want(group, b))


@pytest.mark.parametrize("waves", ["3", "4"])
def test_row_bubble_in_the_second_round(gpu_ctx, monkeypatch, waves):
    monkeypatch.setenv("CL_LANE_MIN_SWEEP", "0")
    monkeypatch.setenv("CL_LANE_WAVES", waves)
    b = _batch(_cases_rounds())
    plan = gpu_ctx.plan(b)
    assert "popoa_lane_kernel<%s>" % waves in [li["kernel"] for li in plan.launches() if li["n_problems"]], plan.launches()
    plan.destroy()
    _check(gpu_ctx, monkeypatch, b, _want("rounds", b))


def test_row_bubble_in_a_wide_pair(gpu_ctx, monkeypatch):
    monkeypatch.setenv("CL_LANE_MIN_SWEEP", "0")
    monkeypatch.setenv("CL_LANE_WIDE", "1")
    b = _batch(_cases_rounds())
    _check(gpu_ctx, monkeypatch, b, _want("rounds", b), kernel="popoa_lane_kernel<4, wide>")


def _mixed_cases():
    return [_cases_rows()[1], _cases_rows()[3], _cases_cols()[2], _cases_cols()[7], _cases_both()[0], _cases_sources()[3], _cases_distances()[2], _cases_saved_columns()[1]]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("npw", [1, 2, 3])
def test_both_orientations_every_num_pw(gpu_ctx, monkeypatch, npw, swap):
    monkeypatch.setenv("CL_LANE_MIN_SWEEP", "0")
    b = _batch(_mixed_cases(), swap=swap)
    f = np.full(b.n_problems, npw, np.uint8)
    _check(gpu_ctx, monkeypatch, b, _want(("npw", npw, swap), b, force_num_pw=f), force_num_pw=f)
    tp = H.tie_params()
    _check(gpu_ctx, monkeypatch, b, _want(("ties", npw, swap), b, force_num_pw=f, params=tp), force_num_pw=f, params=tp)


def test_through_the_narrow_launch(gpu_ctx, monkeypatch):
    monkeypatch.setenv("CL_LANE_MIN_SWEEP", "0")
    short_rows = [Case("one_wave_row_bubble", dict(n=40, seed=50, snps=[20]), dict(n=C, seed=51)), Case("one_wave_col_bubble", dict(n=50, seed=52), dict(n=C, seed=53, snps=[70], dels=[(100, 2)]))]
    head = _batch(_mixed_cases() + short_rows)
    rng = np.random.default_rng(54)
    fill = synth.linear_batch([(int(rng.integers(3, 12)), int(rng.integers(3, 16))) for _ in range(2060 - head.n_problems)], seed=55)
    b = capi.StitchBatch.concat([head, fill])
    assert b.n_problems >= 2048
    _check(gpu_ctx, monkeypatch, b, _want("narrow", b), kernel="popoa_narrow_kernel")
