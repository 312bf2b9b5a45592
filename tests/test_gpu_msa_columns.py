"""The MSA as columns on the device: cl_msa_columns_compute (msa_columns_kernels.hip) against the host definition cl_msa_columns_host on the
committed MSA graphs and on crafted paths — block seams, row counts around a wave, column counts around the reduce kernel's four columns a
thread and 256 threads a workgroup, sites carried across workgroups and blocks, 65 541 paths against the 65 535 grid rows over which
msa_fill_kernel strides (and counts beyond 16 bits) —, its error codes, and the command line's --msa-out,
--column-stats and --variable-sites.  Every comparison is exact."""
import numpy as np
import pytest

from centrolign_amd import capi
from tests import test_gpu_induced_pairs as tip
from tests import test_msa_columns as tmc

ARRAYS = ("node_col", "rows", "columns", "site_col", "site_rows")


def device_or_code(ctx, g, **kw):
    try:
        return capi.msa_columns(g, ctx, **kw)
    except capi.ClError as e:
        return e.code


def same_as_host(got, host, want=7, what=""):
    """the wanted arrays are the host's byte for byte, the others absent"""
    wanted = {"node_col": True, "rows": want & 1, "columns": want & 2, "site_col": want & 4, "site_rows": want & 4}
    assert got["n_paths"] == host["n_paths"] and got["n_cols"] == host["n_cols"], what
    assert got["n_sites"] == (host["n_sites"] if want & 4 else 0), what
    for k in ARRAYS:
        if not wanted[k]:
            assert got[k] is None, (what, k)
        else:
            assert got[k] is not None and got[k].shape == host[k].shape and got[k].dtype == host[k].dtype and np.array_equal(got[k], host[k]), (what, k)


def msa_like(seed, backbone=1500, n_paths=5, snp_run=(200, 330), indels_from=400, snp_p=0.1, indel_p=0.01, long_insertion=(700, 600)):
    """a backbone every path follows, with SNP bubbles (every position of snp_run, and at random behind indels_from), short deletions and
    insertions behind indels_from, and one long insertion private to path 0: in level layout the columns up to indels_from are the backbone's"""
    rng = np.random.default_rng(seed)
    labels = [int(b) for b in rng.integers(0, 4, backbone)]
    alt = {}
    for i in range(backbone):
        if snp_run[0] <= i < snp_run[1] or (i >= indels_from and rng.random() < snp_p):
            alt[i] = len(labels)
            labels.append((labels[i] + 1 + int(rng.integers(0, 3))) % 4)
    paths = []
    for p in range(n_paths):
        path, i = [], 0
        while i < backbone:
            if i >= indels_from and rng.random() < indel_p:
                i += int(rng.integers(1, 8))
                continue
            take_alt = i in alt and (rng.random() < 0.4 if p > 1 or not snp_run[0] <= i < snp_run[1] else p == 0)   # paths 0 and 1 differ all along snp_run
            path.append(alt[i] if take_alt else i)
            fresh = 0
            if i >= indels_from and rng.random() < indel_p:
                fresh = int(rng.integers(1, 6))
            if p == 0 and long_insertion and i == long_insertion[0]:
                fresh = long_insertion[1]
            path += range(len(labels), len(labels) + fresh)
            labels += [int(b) for b in rng.integers(0, 4, fresh)]
            i += 1
        paths.append(path)
    return tip.path_graph(labels, paths)


@pytest.mark.gpu
def test_gpu_equals_host_on_msa_graphs(gpu_ctx):
    """both layouts and every combination of what is wanted; what is not wanted does not come back"""
    seen = 0
    for name, g in tmc.golden().items():
        for layout in tmc.LAYOUTS:
            host = capi.msa_columns_host(g, layout=layout)
            for want in range(8):
                same_as_host(capi.msa_columns(g, gpu_ctx, layout=layout, want=want), host, want, (name, layout, want))
                seen += 1
    assert seen >= 64


@pytest.mark.gpu
def test_gpu_block_seams(gpu_ctx):
    """one graph under block widths 1, 3, 256, n_cols - 1, n_cols, n_cols + 1 and the default: a block in which four of the five paths have no
    step (inside path 0's long insertion), widths that are no multiple of 4, sites on both sides of a seam, a seam inside a run of sites"""
    g = msa_like(11)
    for layout in tmc.LAYOUTS:
        host = capi.msa_columns_host(g, layout=layout)
        W = host["n_cols"]
        if layout == "level":
            sites = set(host["site_col"].tolist())
            assert set(range(200, 330)) <= sites                                   # the run of sites over the seam at 256 (and every seam at 1 and 3)
            assert any(s > 1024 for s in sites) and host["n_sites"] > 200
            cols = [host["node_col"][g.path_nodes[int(g.path_off[p]):int(g.path_off[p + 1])]] for p in range(5)]
            empty = [b for b in range(W // 256) if any(not np.any((c >= 256 * b) & (c < 256 * b + 256)) for c in cols)]
            assert empty, "no block of 256 columns without a step of some path"
        assert W > 2000
        for block_cols in (1, 3, 256, 257, W - 1, W, W + 1, None):
            same_as_host(capi.msa_columns(g, gpu_ctx, layout=layout, block_cols=block_cols), host, 7, (layout, block_cols))
        for want in (1, 2, 4, 6):
            same_as_host(capi.msa_columns(g, gpu_ctx, layout=layout, block_cols=257, want=want), host, want, (layout, want))
    two = capi.msa_columns_host(g, min_minor=2, max_gaps=1)
    assert 0 < two["n_sites"] < capi.msa_columns_host(g)["n_sites"]
    same_as_host(capi.msa_columns(g, gpu_ctx, min_minor=2, max_gaps=1, block_cols=100), two, 7, "thresholds")


@pytest.mark.gpu
@pytest.mark.parametrize("n_paths", [1, 2, 63, 64, 65, 130])
def test_gpu_row_counts_around_a_wave(gpu_ctx, n_paths):
    g = msa_like(20 + n_paths, backbone=300, n_paths=n_paths, snp_run=(10, 40), indels_from=60, snp_p=0.2, indel_p=0.02, long_insertion=None)
    for layout in tmc.LAYOUTS:
        host = capi.msa_columns_host(g, layout=layout)
        assert host["n_cols"] >= 280 and host["n_paths"] == n_paths   # (about 300: the backbone, less a deletion or two, plus insertions)
        for block_cols in (None, 100):
            same_as_host(capi.msa_columns(g, gpu_ctx, layout=layout, block_cols=block_cols), host, 7, (layout, block_cols))


def many_paths_graph(P, W):
    """P paths over a backbone of W columns with a SNP alternate in every column but the first and deletions of one to three columns from the
    sixth on; numpy all the way (msa_like's loops take a second per thousand paths)"""
    rng = np.random.default_rng(P)
    labels = rng.integers(0, 4, W)
    labels = np.concatenate([labels, (labels + rng.integers(1, 4, W)) % 4])   # node W + i: the other base of column i
    alt = rng.random((P, W)) < 0.3
    alt[:, 0] = False
    start, length = rng.random((P, W)) < 0.02, rng.integers(1, 4, (P, W))
    start[:, :5] = False
    deleted = np.zeros((P, W), bool)
    for s in range(3):
        deleted[:, s:] |= (start & (length > s))[:, :W - s]
    nodes = np.where(alt, W + np.arange(W), np.arange(W))
    off = np.concatenate([[0], np.cumsum((~deleted).sum(1))]).astype(np.uint64)
    z = np.zeros(2 * W + 1, np.uint64)
    assert np.any(deleted)
    return capi.BaseGraph(labels.astype(np.uint8), z, np.zeros(0, np.uint32), z, np.zeros(0, np.uint32), off, nodes[~deleted].astype(np.uint32), 0, 0)


@pytest.mark.gpu
def test_gpu_more_paths_than_grid_rows(gpu_ctx):
    """65 541 paths over 40 columns: msa_fill_kernel's grid has 65 535 rows, so rows 0 .. 5 walk a second path each; and a column holds more
    than 65 535 bases"""
    P, W = 65541, 40
    g = many_paths_graph(P, W)
    assert len(g.path_off) - 1 == P > 65535 and int(g.path_off[-1]) > 2500000
    for layout in tmc.LAYOUTS:
        host = capi.msa_columns_host(g, layout=layout)
        assert host["n_paths"] == P and host["n_cols"] == (W if layout == "level" else 2 * W - 1)   # (column 0 has no alternate)
        assert int(host["columns"][:, :5].sum(1).max()) > 65535 and int(host["columns"][:, :4].max()) > 65535   # (no 16-bit count holds these)
        if layout == "level":
            assert host["n_sites"] > 30 and np.any(host["columns"][:, 5] > 0)
        for block_cols in (None, 16):
            same_as_host(capi.msa_columns(g, gpu_ctx, layout=layout, want=7, block_cols=block_cols), host, 7, (layout, block_cols))


@pytest.mark.gpu
@pytest.mark.parametrize("n_cols", [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025])
def test_gpu_column_counts_around_the_vector_width_and_the_workgroup(gpu_ctx, n_cols):
    g = msa_like(40 + n_cols, backbone=n_cols, n_paths=3, snp_run=(0, 0), indels_from=0, snp_p=0.3, indel_p=0.0, long_insertion=None)
    host = capi.msa_columns_host(g)
    assert host["n_cols"] == n_cols
    same_as_host(capi.msa_columns(g, gpu_ctx), host)
    same_as_host(capi.msa_columns(g, gpu_ctx, layout="node"), capi.msa_columns_host(g, layout="node"))


@pytest.mark.gpu
def test_gpu_sites_none_all_and_more_than_a_workgroup(gpu_ctx):
    n = 1500
    rng = np.random.default_rng(3)
    labels = [int(b) for b in rng.integers(0, 4, n)]
    none = tip.path_graph(labels, [list(range(n))] * 3)
    host = capi.msa_columns_host(none)
    assert host["n_sites"] == 0
    same_as_host(capi.msa_columns(none, gpu_ctx, block_cols=700), host)
    # every column a two-branch bubble: 1 500 sites, more than the 256 columns of a workgroup and than a block of 700 columns
    every = tip.path_graph(labels + [(b + 1) % 4 for b in labels], [list(range(n)), list(range(n, 2 * n)), list(range(n))])
    host = capi.msa_columns_host(every)
    assert host["n_cols"] == n and host["site_col"].tolist() == list(range(n))
    for block_cols in (700, 256, None):
        got = capi.msa_columns(every, gpu_ctx, block_cols=block_cols)
        same_as_host(got, host, 7, block_cols)
        assert got["site_col"].tolist() == list(range(n))
    same_as_host(capi.msa_columns(every, gpu_ctx, block_cols=700, want=4), host, 4)
    # sites here and there: the offsets of workgroups with and without sites
    some = msa_like(5, backbone=3000, n_paths=4, snp_run=(500, 500), indels_from=0, snp_p=0.02, indel_p=0.0, long_insertion=None)
    host = capi.msa_columns_host(some)
    assert 10 < host["n_sites"] < 200
    for block_cols in (None, 1000, 255):
        same_as_host(capi.msa_columns(some, gpu_ctx, block_cols=block_cols), host, 7, block_cols)


@pytest.mark.gpu
def test_gpu_crafted_paths_and_thresholds(gpu_ctx):
    for name, (g, rows, node_col) in tmc.crafted_cases().items():
        for layout in tmc.LAYOUTS:
            got = capi.msa_columns(g, gpu_ctx, layout=layout)
            assert tmc.text(got["rows"]) == rows[layout] and got["node_col"].tolist() == node_col[layout], (name, layout)
            same_as_host(got, capi.msa_columns_host(g, layout=layout), 7, (name, layout))
    g = tmc.threshold_graph()
    for kw in ({}, {"min_minor": 2}, {"max_gaps": 0}, {"min_minor": 2, "max_gaps": 1}, {"min_minor": 3}):
        for block_cols in (None, 2):
            same_as_host(capi.msa_columns(g, gpu_ctx, block_cols=block_cols, **kw), capi.msa_columns_host(g, **kw), 7, kw)
    assert tmc.text(capi.msa_columns(g, gpu_ctx)["site_rows"]) == [b"AA-", b"AAC", b"GAC", b"GGG"]


@pytest.mark.gpu
def test_gpu_error_codes_are_the_hosts(gpu_ctx):
    for name, (g, kw, code) in tmc.error_cases().items():
        assert device_or_code(gpu_ctx, g, **kw) == code == tmc.host_or_code(g, **kw), name
    # the context is as good as before
    g = tmc.threshold_graph()
    same_as_host(capi.msa_columns(g, gpu_ctx), capi.msa_columns_host(g))


def fasta_entries(text):
    lines = text.decode().split("\n")
    assert lines[-1] == "" and len(lines) % 2 == 1 and all(ln.startswith(">") for ln in lines[0:-1:2])
    return [ln[1:] for ln in lines[0:-1:2]], [ln.encode() for ln in lines[1:-1:2]]


@pytest.mark.gpu
def test_gpu_cli_msa_files(gpu_ctx, tmp_path):
    """--msa-out, --column-stats and --variable-sites in one run, under both layouts and under other site thresholds: the files are the host
    function's results on the graph the run printed, every aligned row degapped is its input sequence, and standard output is what it is without
    the options.  The three 6 kbp sequences of test_gpu_cli.py's smallest MSA: four short runs of the tool."""
    from centrolign_amd import synth
    from tests import helpers as H
    from tests import test_gpu_cli as tgc
    case = [c for c in H.msa_cases() if c[0] == "msa3_6k"][0]
    fa, nwk, budget, printed = tgc.msa_case(tmp_path, case)
    seqs = synth.hor_sequences(case[3], case[2], case[1], seq_div=0.01, hor_div=0.03, indel_hor=2)
    names = ["seq%d" % i for i in range(case[1])]
    base = ["-v", 0, "-T", nwk, "-a", budget]
    plain = tgc.run(base + [fa], tmp_path)
    assert plain.stdout == printed and printed.startswith(b"H\t")
    g, path_names = capi.read_gfa(plain.stdout)
    assert sorted(path_names) == names
    runs = (("level", {}, ["--msa-out", "--column-stats", "--variable-sites"], []),
            ("node", {}, ["--msa-out", "--column-stats", "--variable-sites"], ["--msa-layout", "node"]),
            ("level", {"min_minor": 2, "max_gaps": 0}, ["--column-stats", "--variable-sites"], ["--msa-layout", "level", "--site-min-minor", 2, "--site-max-gaps", 0]))
    for k, (layout, kw, files, extra) in enumerate(runs):
        file_of = {opt: "%d%s" % (k, opt.replace("--", ".")) for opt in files}
        got = tgc.run(base + [x for opt in files for x in (opt, file_of[opt])] + extra + [fa], tmp_path)
        assert got.stdout == plain.stdout
        host = capi.msa_columns_host(g, layout=layout, **kw)
        if "--msa-out" in files:
            entry_names, rows = fasta_entries((tmp_path / file_of["--msa-out"]).read_bytes())
            assert entry_names == path_names and rows == tmc.text(host["rows"])
            for nm, row in zip(entry_names, rows):
                assert row.replace(b"-", b"").decode() == seqs[names.index(nm)], nm
        lines = (tmp_path / file_of["--column-stats"]).read_text().split("\n")
        assert lines[0].split("\t") == "column A C G T N gaps consensus site".split() and lines[-1] == ""
        want = [[str(c)] + [str(v) for v in r[:6]] + ["ACGTN-"[r[6]], str(r[7] & 1)] for c, r in enumerate(host["columns"].tolist())]
        assert [ln.split("\t") for ln in lines[1:-1]] == want
        entry_names, site_rows = fasta_entries((tmp_path / file_of["--variable-sites"]).read_bytes())
        assert entry_names == path_names and site_rows == tmc.text(host["site_rows"])
        assert [c for c, ln in enumerate(lines[1:-1]) if ln.endswith("\t1")] == host["site_col"].tolist()
        assert (host["n_sites"] > 0) == (k == 0) or k == 2   # sites in the level layout; none can exist with one node per column
    # -c with any of the three is refused before anything runs
    for opt in ("--msa-out", "--column-stats", "--variable-sites"):
        r = tmc.run(base + [opt, "refused.out", "-c", fa], tmp_path)
        assert tmc.refused(r) and "-c" in r.stderr.decode(), opt
    assert not (tmp_path / "refused.out").exists()
