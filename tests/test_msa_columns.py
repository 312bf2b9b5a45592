"""The MSA as columns on the host: cl_msa_column_layout and cl_msa_columns_host (cl_columns_api.cpp) against a numpy restatement written
independently of the C++ (Kahn over the path edges, a scatter, np.bincount), against literal bytes on crafted paths, their error codes, and the
command line's option checks that need no device.  Every comparison is exact."""
import os

import numpy as np
import pytest

from centrolign_amd import capi
from tests import test_cli
from tests import test_gpu_induced_pairs as tip

NO = capi.NO_COLUMN
LAYOUTS = ("level", "node")
A, Cc, G, T, N = range(5)


# ---------------------------------------------------------------- the restatement ------------------------------------------------------------
def path_edges(g):
    """the distinct (tail, head) of consecutive steps of every path"""
    nodes, off = g.path_nodes.astype(np.int64), g.path_off.astype(np.int64)
    if len(nodes) < 2:
        return np.zeros((0, 2), np.int64)
    inside = np.ones(len(nodes) - 1, bool)       # step i and i + 1 lie on one path
    starts = off[1:-1]
    inside[starts[(starts > 0) & (starts < len(nodes))] - 1] = False
    return np.unique(np.stack([nodes[:-1][inside], nodes[1:][inside]], 1), axis=0)


def levels(g):
    """level per node (-1: on no path) by Kahn's algorithm, or None if the path edges have a cycle"""
    n = len(g.label)
    used = np.zeros(n, bool)
    used[g.path_nodes] = True
    e = path_edges(g)
    indeg = np.bincount(e[:, 1], minlength=n)
    first = np.searchsorted(e[:, 0], np.arange(n + 1))   # (np.unique sorted the rows by tail)
    heads, indeg, first = e[:, 1].tolist(), indeg.tolist(), first.tolist()
    level = [0] * n
    todo = [v for v in np.flatnonzero(used).tolist() if indeg[v] == 0]
    done = 0
    while todo:
        u = todo.pop()
        done += 1
        for v in heads[first[u]:first[u + 1]]:
            if level[v] < level[u] + 1:
                level[v] = level[u] + 1
            indeg[v] -= 1
            if indeg[v] == 0:
                todo.append(v)
    if done != int(used.sum()):
        return None
    return np.where(used, np.asarray(level, np.int64), -1)


def restate(g, layout, min_minor=1, max_gaps=0xFFFFFFFF):
    level = levels(g)
    assert level is not None, "the path edges have a cycle"
    n, P = len(g.label), len(g.path_off) - 1
    used = np.flatnonzero(level >= 0)
    col = np.full(n, NO, np.int64)
    if layout == "level":
        col[used] = level[used]
        W = int(level.max()) + 1 if len(used) else 0
    else:
        col[used[np.lexsort((used, level[used]))]] = np.arange(len(used))
        W = len(used)
    nodes = g.path_nodes.astype(np.int64)
    row_of = np.repeat(np.arange(P), np.diff(g.path_off.astype(np.int64)))
    rows = np.full((P, W), b"-", "S1")
    rows[row_of, col[nodes]] = np.array(list("ACGTN"), "S1")[g.label[nodes]]
    count = np.bincount(col[nodes] * 5 + g.label[nodes], minlength=5 * W).reshape(W, 5)
    gaps = P - count.sum(1)
    consensus = np.argmax(np.concatenate([count, gaps[:, None]], 1), 1) if W else np.zeros(0, np.int64)   # (argmax: the first of the largest)
    second = np.sort(count[:, :4], 1)[:, 2]
    flags = ((second >= min_minor) & (gaps <= max_gaps)) * 1 + (gaps > 0) * 2 + (count[:, 4] > 0) * 4
    sites = np.flatnonzero(flags & 1)
    return {"n_paths": P, "n_cols": W, "n_sites": len(sites), "node_col": col.astype(np.uint32), "rows": rows,
            "columns": np.concatenate([count, gaps[:, None], consensus[:, None], flags[:, None]], 1).astype(np.uint32).reshape(W, 8),
            "site_col": sites.astype(np.uint64), "site_rows": rows[:, sites]}


KEYS = ("n_paths", "n_cols", "n_sites", "node_col", "rows", "columns", "site_col", "site_rows")


def same(got, want, what=""):
    for k in KEYS:
        if isinstance(want[k], int):
            assert got[k] == want[k], (what, k, got[k], want[k])
        else:
            assert got[k] is not None and got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)


def text(rows):
    return [b"".join(r) for r in rows.tolist()] if rows.size else [b""] * rows.shape[0]


def host_or_code(g, **kw):
    try:
        return capi.msa_columns_host(g, **kw)
    except capi.ClError as e:
        return e.code


_golden = {}


def golden():
    """the committed MSA graphs, read once"""
    if not _golden:
        _golden.update(tip.golden_graphs())
    return _golden


# ---------------------------------------------------------------- crafted paths ---------------------------------------------------------------
def crafted_cases():
    """name -> (graph, {layout: rows as bytes}, {layout: node_col})"""
    pg = tip.path_graph
    return {
        "one path": (pg([A, Cc, G], [[0, 1, 2]]), {"level": [b"ACG"], "node": [b"ACG"]}, {"level": [0, 1, 2], "node": [0, 1, 2]}),
        "two identical paths": (pg([A, Cc, G], [[0, 1, 2], [0, 1, 2]]), {"level": [b"ACG", b"ACG"], "node": [b"ACG", b"ACG"]},
                                {"level": [0, 1, 2], "node": [0, 1, 2]}),
        # node 1 (A) and node 2 (G) are the two branches of a SNP bubble
        "snp bubble": (pg([A, A, G, T], [[0, 1, 3], [0, 2, 3]]), {"level": [b"AAT", b"AGT"], "node": [b"AA-T", b"A-GT"]},
                       {"level": [0, 1, 1, 2], "node": [0, 1, 2, 3]}),
        # branches of 3 (C) and 5 (G) nodes between A and T: left-justified against one another
        "3 against 5": (pg([A, Cc, Cc, Cc, G, G, G, G, G, T], [[0, 1, 2, 3, 9], [0, 4, 5, 6, 7, 8, 9]]),
                        {"level": [b"ACCC--T", b"AGGGGGT"], "node": [b"AC-C-C---T", b"A-G-G-GGGT"]},
                        {"level": [0, 1, 2, 3, 1, 2, 3, 4, 5, 6], "node": [0, 1, 3, 5, 2, 4, 6, 7, 8, 9]}),
        "insertion on one path": (pg([A, Cc, G, T], [[0, 1, 3], [0, 1, 2, 3]]), {"level": [b"AC-T", b"ACGT"], "node": [b"AC-T", b"ACGT"]},
                                  {"level": [0, 1, 2, 3], "node": [0, 1, 2, 3]}),
        "an empty path": (pg([A, Cc], [[0, 1], []]), {"level": [b"AC", b"--"], "node": [b"AC", b"--"]}, {"level": [0, 1], "node": [0, 1]}),
        "a node on no path": (pg([A, Cc, G, T], [[0, 2]]), {"level": [b"AG"], "node": [b"AG"]}, {"level": [0, NO, 1, NO], "node": [0, NO, 1, NO]}),
        "no paths": (pg([A, Cc], []), {"level": [], "node": []}, {"level": [NO, NO], "node": [NO, NO]}),
    }


@pytest.mark.parametrize("name", list(crafted_cases()))
def test_crafted_paths_give_these_bytes(name):
    g, rows, node_col = crafted_cases()[name]
    for layout in LAYOUTS:
        got = capi.msa_columns_host(g, layout=layout)
        assert text(got["rows"]) == rows[layout], layout
        assert got["node_col"].tolist() == node_col[layout], layout
        assert got["n_cols"] == (len(rows[layout][0]) if rows[layout] else 0) and got["n_paths"] == len(rows[layout])
        assert got["rows"].shape == (got["n_paths"], got["n_cols"]) and got["columns"].shape == (got["n_cols"], 8)
        same(got, restate(g, layout), (name, layout))
        col, n_cols = capi.msa_column_layout(g, layout)
        assert col.tolist() == node_col[layout] and n_cols == got["n_cols"]


def test_the_snp_column_and_the_gap_columns():
    g = crafted_cases()["snp bubble"][0]
    level, node = capi.msa_columns_host(g, layout="level"), capi.msa_columns_host(g, layout="node")
    #                               A  C  G  T  N  gaps consensus flags
    assert level["columns"].tolist() == [[2, 0, 0, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0, 1], [0, 0, 0, 2, 0, 0, 3, 0]]
    assert level["site_col"].tolist() == [1] and text(level["site_rows"]) == [b"A", b"G"]
    assert node["columns"].tolist() == [[2, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 1, 0, 2], [0, 0, 1, 0, 0, 1, 2, 2], [0, 0, 0, 2, 0, 0, 3, 0]]
    assert node["n_sites"] == 0 and node["site_col"].shape == (0,) and node["site_rows"].shape == (2, 0)


def test_consensus_ties_go_to_the_first_of_acgtn_gap():
    # column 0: A = C -> A; column 1: G = N -> G; column 2: N = the gap -> N
    g = tip.path_graph([A, Cc, G, N, N], [[0, 2, 3], [1, 4]])
    got = capi.msa_columns_host(g, layout="level")
    assert text(got["rows"]) == [b"AGN", b"CN-"]
    assert got["columns"].tolist() == [[1, 1, 0, 0, 0, 0, 0, 1], [0, 0, 1, 0, 1, 0, 2, 4], [0, 0, 0, 0, 1, 1, 4, 6]]
    # an all-N column (two N nodes side by side), and a column where the gap alone is the largest
    g = tip.path_graph([A, N, N, G], [[0, 1], [0, 2], [0, 1, 3]])
    got = capi.msa_columns_host(g, layout="level")
    assert text(got["rows"]) == [b"AN-", b"AN-", b"ANG"]
    assert got["columns"].tolist() == [[3, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 3, 0, 4, 4], [0, 0, 1, 0, 0, 2, 5, 2]]
    # a base = the gap -> the base
    got = capi.msa_columns_host(crafted_cases()["insertion on one path"][0])
    assert got["columns"][2].tolist() == [0, 0, 1, 0, 0, 1, 2, 2]


def threshold_graph():
    """rows AAA-T / AAACT / AGACT / AGGGT: a 2 + 2 column, a 3 + 1 column, a column C C G gap"""
    return tip.path_graph([A, A, G, A, G, Cc, T, G], [[0, 1, 3, 6], [0, 1, 3, 5, 6], [0, 2, 3, 5, 6], [0, 2, 4, 7, 6]])


def test_site_thresholds():
    g = threshold_graph()
    got = capi.msa_columns_host(g)
    assert text(got["rows"]) == [b"AAA-T", b"AAACT", b"AGACT", b"AGGGT"]
    assert got["columns"][:, :6].tolist() == [[4, 0, 0, 0, 0, 0], [2, 0, 2, 0, 0, 0], [3, 0, 1, 0, 0, 0], [0, 2, 1, 0, 0, 1], [0, 0, 0, 4, 0, 0]]
    assert got["columns"][:, 7].tolist() == [0, 1, 1, 3, 0]
    assert got["site_col"].tolist() == [1, 2, 3] and text(got["site_rows"]) == [b"AA-", b"AAC", b"GAC", b"GGG"]
    two = capi.msa_columns_host(g, min_minor=2)
    assert two["site_col"].tolist() == [1] and text(two["site_rows"]) == [b"A", b"A", b"G", b"G"] and two["columns"][:, 7].tolist() == [0, 1, 0, 2, 0]
    full = capi.msa_columns_host(g, max_gaps=0)
    assert full["site_col"].tolist() == [1, 2] and text(full["site_rows"]) == [b"AA", b"AA", b"GA", b"GG"]
    assert capi.msa_columns_host(g, min_minor=3)["n_sites"] == 0
    for kw in ({}, {"min_minor": 2}, {"max_gaps": 0}, {"min_minor": 2, "max_gaps": 1}):
        for layout in LAYOUTS:
            same(capi.msa_columns_host(g, layout=layout, **kw), restate(g, layout, **{"min_minor": 1, "max_gaps": 0xFFFFFFFF, **kw}), (kw, layout))
    one = capi.msa_columns_host(tip.path_graph([A, Cc, G], [[0, 1, 2]]))   # one path: no column has a second base
    assert one["n_sites"] == 0 and one["columns"][:, 7].tolist() == [0, 0, 0]


def test_want_selects_the_arrays():
    g = threshold_graph()
    everything = capi.msa_columns_host(g)
    for want in range(8):
        got = capi.msa_columns_host(g, want=want)
        assert np.array_equal(got["node_col"], everything["node_col"]) and got["n_cols"] == 5
        for bit, keys in ((1, ("rows",)), (2, ("columns",)), (4, ("site_col", "site_rows"))):
            for k in keys:
                assert (got[k] is None) if not want & bit else np.array_equal(got[k], everything[k]), (want, k)
        assert got["n_sites"] == (3 if want & 4 else 0)
    assert capi.msa_columns_host(g, want=capi.MSA_WANT_ROWS | capi.MSA_WANT_SITES)["columns"] is None


# ---------------------------------------------------------------- the committed MSA graphs ---------------------------------------------------
def check_properties(g, got, layout):
    P = len(g.path_off) - 1
    dec = np.array(list("ACGTN"), "S1")
    for p in range(P):
        steps = g.path_nodes[int(g.path_off[p]):int(g.path_off[p + 1])]
        row = got["rows"][p]
        assert np.array_equal(row[row != b"-"], dec[g.label[steps]]), p                  # degapped: the path's sequence
        assert np.all(np.diff(got["node_col"][steps].astype(np.int64)) > 0), p           # columns strictly increase along a path
    assert np.all(got["columns"][:, :6].sum(1) == P)
    if layout == "node":
        used = np.unique(g.path_nodes)
        assert got["n_cols"] == len(used)
        assert np.array_equal(np.sort(got["node_col"][used]), np.arange(len(used)))      # every column holds one node
    unused = np.ones(len(g.label), bool)
    unused[g.path_nodes] = False
    assert np.all(got["node_col"][unused] == NO)


def test_host_equals_the_restatement_on_msa_graphs():
    seen = 0
    for name, g in golden().items():
        for layout in LAYOUTS:
            got = capi.msa_columns_host(g, layout=layout)
            same(got, restate(g, layout), (name, layout))
            check_properties(g, got, layout)
            col, n_cols = capi.msa_column_layout(g, layout)
            assert np.array_equal(col, got["node_col"]) and n_cols == got["n_cols"]
            seen += 1
    assert seen >= 8


def test_cross_checked_column_counts():
    """values computed with a separate prototype (level layout)"""
    graphs = golden()
    wide = graphs["wide_merge_50x5k"]
    assert len(wide.label) == 243624 + 2 and len(wide.path_off) - 1 == 50   # (read_gfa adds the two sentinels, which lie on no path)
    assert capi.msa_column_layout(wide, "node")[1] == len(np.unique(wide.path_nodes)) == 243624
    assert capi.msa_column_layout(wide, "level")[1] == 7061
    assert capi.msa_column_layout(graphs["msa_text:msa4_8k"], "level")[1] == 12091
    assert capi.msa_column_layout(graphs["msa_text:msa3_6k"], "level")[1] == 6005


# ---------------------------------------------------------------- error codes -----------------------------------------------------------------
def error_cases():
    """name -> (graph, parameters, code)"""
    pg = tip.path_graph
    fine = pg([A, Cc, G, T], [[0, 1, 2], [0, 2, 3]])
    out_of_range = pg([A, Cc, G, T], [[0, 1, 2], [0, 2, 3]])
    out_of_range.path_nodes[4] = 1000
    return {
        "a path repeats a node": (pg([A, Cc, G], [[0, 1, 2, 1]]), {}, -7),
        "a path repeats a node at once": (pg([A, Cc, G], [[0, 1, 1, 2]]), {}, -7),
        "two paths in opposite order": (pg([A, Cc, G], [[0, 1, 2], [2, 0]]), {}, -7),
        "label 5 on a path": (pg([A, 5, G], [[0, 1, 2]]), {}, -1),
        "min_minor 0": (fine, {"min_minor": 0}, -1),
        "layout 2": (fine, {"layout": 2}, -1),
        "unknown want bit": (fine, {"want": 8}, -1),
        "node id out of range": (out_of_range, {}, -1),
    }


@pytest.mark.parametrize("name", list(error_cases()))
def test_error_codes(name):
    g, kw, code = error_cases()[name]
    assert host_or_code(g, **kw) == code
    if not kw or "layout" in kw:
        if name != "label 5 on a path":   # (the layout reads no label)
            with pytest.raises(capi.ClError) as e:
                capi.msa_column_layout(g, kw.get("layout", "level"))
            assert e.value.code == code


def test_label_5_off_the_paths_is_fine():
    got = capi.msa_columns_host(tip.path_graph([A, 5, G, 6], [[0, 2]]))
    assert text(got["rows"]) == [b"AG"]


def test_the_new_symbols_are_exported():
    lib = capi.load_library()
    for sym in ("cl_msa_columns_params_default", "cl_msa_column_layout", "cl_msa_columns_host", "cl_msa_columns_compute", "cl_msa_columns_free",
                "cl_msa_columns_layout_seconds"):
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    import ctypes as C
    assert C.sizeof(capi.MsaColumnsParams) == 24 and C.sizeof(capi.MsaColumnsC) == 64 and len(capi.MSA_COLUMN_FIELDS) == 8
    p = capi.MsaColumnsParams()
    lib.cl_msa_columns_params_default(C.byref(p))
    assert (p.layout, p.want, p.min_minor, p.max_gaps, p.block_cols) == (0, 7, 1, 0xFFFFFFFF, 0)
    capi.msa_columns_host(threshold_graph())
    assert 0.0 <= capi.msa_columns_layout_seconds() < 1.0


# ---------------------------------------------------------------- the command line ------------------------------------------------------------
def run(args, cwd):
    return test_cli.run([str(a) for a in args], cwd=str(cwd))


def refused(r):
    lines = r.stderr.decode().splitlines()
    return r.returncode == 1 and r.stdout == b"" and len(lines) == 1 and lines[0].startswith("error: ")


def test_cli_refuses_before_reading_anything(tmp_path):
    """none of these names an input that exists: a refusal that came after reading the FASTA would be a different message"""
    existing = tmp_path / "kept.txt"
    existing.write_text("kept\n")
    three = ("--msa-out", "--column-stats", "--variable-sites")
    cases = [[opt, existing, "missing.fa"] for opt in three]
    cases += [[a, "same.out", b, "same.out", "missing.fa"] for a in three for b in three if a < b]
    for other in ("--pair-stats", "--dist-out", "--pair-profile", "--pair-events", "--tree-out", "-s"):
        cases.append(["--msa-out", "same.out", other, "same.out", "--infer-tree", "missing.fa"])
    cases.append(["--column-stats", "same.out", "--compare-to", "base.gfa", "--pair-agreement", "same.out", "missing.fa"])
    cases += [[opt, "new.out", "-c", "missing.fa"] for opt in three]
    cases += [["--msa-layout", "node", "missing.fa"], ["--site-min-minor", "2", "missing.fa"], ["--site-max-gaps", "0", "missing.fa"],
              ["--site-min-minor", "2", "--msa-out", "m.fa", "missing.fa"], ["--site-max-gaps", "2", "--msa-out", "m.fa", "missing.fa"]]
    cases += [["--msa-out", "m.fa", "--msa-layout", bad, "missing.fa"] for bad in ("levels", "Node", "", "0", "1")]
    for bad in ("0", "-3", "1.5", "ten", "", "+4", "1e3"):
        cases.append(["--column-stats", "c.tsv", "--site-min-minor", bad, "missing.fa"])
        if bad != "0":
            cases.append(["--variable-sites", "v.fa", "--site-max-gaps", bad, "missing.fa"])
    for args in cases:
        r = run(args, tmp_path)
        assert refused(r), (args, r.stderr)
        assert "missing.fa" not in r.stderr.decode(), args
        assert sorted(os.listdir(tmp_path)) == ["kept.txt"], args
    assert existing.read_text() == "kept\n"
    # accepted: the run gets as far as the missing FASTA
    for args in (["--msa-out", "m.fa", "--msa-layout", "node"], ["--msa-out", "m.fa", "--column-stats", "c.tsv", "--variable-sites", "v.fa", "--msa-layout", "level"],
                 ["--column-stats", "c.tsv", "--site-min-minor", "1", "--site-max-gaps", "0"], ["--variable-sites", "v.fa", "--site-min-minor", "3"]):
        r = run(["-v", "0"] + args + ["missing.fa"], tmp_path)
        assert refused(r) and "missing.fa" in r.stderr.decode(), args
    assert sorted(os.listdir(tmp_path)) == ["kept.txt"]


def test_cli_two_sequences_need_a_graph(tmp_path):
    """refused once the FASTA is read, before a device is opened: without --force-gfa-output two sequences print a CIGAR, no graph"""
    (tmp_path / "in.fa").write_text(">a\nACGTACGT\n>b\nACGAACGT\n")
    for args in (["--msa-out", "m.fa"], ["--column-stats", "c.tsv"], ["--variable-sites", "v.fa"]):
        r = run(["-v", "0"] + args + ["in.fa"], tmp_path)
        assert refused(r) and "--force-gfa-output" in r.stderr.decode(), args
    assert sorted(os.listdir(tmp_path)) == ["in.fa"]


def test_cli_new_options_are_not_parameters(tmp_path):
    base = run(["-G"], tmp_path)
    got = run(["--msa-out", "m.fa", "--column-stats", "c.tsv", "--variable-sites", "v.fa", "--msa-layout", "node", "--site-min-minor", "2", "--site-max-gaps", "3", "-G"], tmp_path)
    assert base.returncode == got.returncode == 0 and got.stdout == base.stdout and got.stderr == b""
    for word in (b"msa-out", b"msa_out", b"column", b"variable", b"layout", b"site"):
        assert word not in got.stdout, word
    assert os.listdir(tmp_path) == []
    h = run(["-h"], tmp_path)
    assert h.returncode == 0
    for opt in ("--msa-out FILE", "--column-stats FILE", "--variable-sites FILE", "--msa-layout WORD", "--site-min-minor INT", "--site-max-gaps INT"):
        assert opt in h.stderr.decode(), opt
    r = run(["--graph", "g.gfa", "--compare-to", "b.gfa", "--pair-agreement", "a.tsv", "--msa-out", "m.fa"], tmp_path)
    assert refused(r) and "--graph" in r.stderr.decode()
