"""Pairwise alignment statistics without a device: cl_induced_pairwise_stat against a parser of cl_induced_pairwise_cigar's text (the texts of
tests/golden/induced_cigars.npz were written by the compiled reference), cl_alignment_distances against the formula of the header restated here,
and the command-line options that are refused before anything is read or opened."""
import gzip
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi
from tests import helpers as H
from tests import test_gpu_induced_pairs as tip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
LETTER = {"=": "eq", "X": "x", "I": "ins", "D": "del"}


def parse_cigar(text):
    """the definition: per letter the sum of the run lengths and the number of runs"""
    out = dict.fromkeys(capi.PAIR_STATS_FIELDS, 0)
    text = text.decode() if isinstance(text, bytes) else str(text)
    runs = re.findall(r"(\d+)([=XID])", text.strip())
    assert "".join(n + c for n, c in runs) == text.strip()
    for n, c in runs:
        out[LETTER[c]] += int(n)
        out[LETTER[c] + "_runs"] += 1
    return out


def stat_or_code(g, a, b):
    try:
        return capi.induced_pairwise_stat(g, a, b)
    except capi.ClError as e:
        return e.code


def crafted_graphs():
    """the crafted-path graphs of test_gpu_induced_pairs.test_gpu_batch_equals_host_on_crafted_paths (same seeds, same order of draws)"""
    rng = np.random.default_rng(9)
    labels = list(rng.integers(0, 4, 64)) + [5, 5, 4, 4]
    base = list(range(40))
    paths = [
        base,
        base[:10] + [50, 51, 52, 53] + base[14:30] + [54, 55, 56, 57, 58] + base[35:],
        [60, 61, 62, 63] + base[4:36] + [50, 51, 52],
        base[20:30] + base[0:10] + base[30:40],
        base[5:8] + base[5:8] + base[0:3],
        [],
        [7],
        [64, 65, 3, 66, 67],
        base[:30] + [41, 42, 43, 44, 45, 46] + base[36:],
        list(range(39, -1, -1)),
        [64, 65, 66, 67],
    ]
    labels += [1] * 200
    paths.append(list(range(68, 268)))
    small = tip.path_graph(labels, paths)
    anc = list(range(30000))
    p2 = [x for x in anc if rng.random() > 0.02]
    p2 = [x if rng.random() > 0.01 else 30000 + int(rng.integers(0, 5000)) for x in p2]
    long = tip.path_graph(rng.integers(0, 4, 100000), [anc, p2, anc[15000:] + anc[:15000], list(range(36000, 100000))])
    return small, long


def check_every_ordered_pair(g):
    n = len(g.path_off) - 1
    for a, b in tip.all_pairs(n):
        want = tip.host_or_code(g, a, b)
        got = stat_or_code(g, a, b)
        assert got == (want if isinstance(want, int) else parse_cigar(want)), (a, b)
    return n * n


def test_stat_equals_the_parsed_reference_cigars():
    z = np.load(os.path.join(H.GOLDEN, "induced_cigars.npz"))
    graphs = {}
    seen = 0
    for key in (str(k) for k in z["keys"]):
        f, a, b = key.split("|")
        if f not in graphs:
            graphs[f] = capi.read_gfa(bytes(z["gfa." + f]))[0]
        want = bytes(z["cigar." + key]) if "cigar." + key in z.files else None
        assert want is not None, key
        assert capi.induced_pairwise_stat(graphs[f], int(a), int(b)) == parse_cigar(want), key
        seen += 1
    assert seen >= 10


def test_stat_equals_the_parsed_cigar_on_the_50_path_root():
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_50x5k.gfa.gz"), "rb").read()))[0]
    assert check_every_ordered_pair(g) == 2500


def test_stat_on_the_crafted_paths():
    small, long = crafted_graphs()
    assert check_every_ordered_pair(small) == 144
    assert check_every_ordered_pair(long) == 16


def test_a_path_against_itself_is_one_match_run():
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_24x7k.gfa.gz"), "rb").read()))[0]
    for p in range(len(g.path_off) - 1):
        n = int(g.path_off[p + 1] - g.path_off[p])
        assert capi.induced_pairwise_stat(g, p, p) == dict(dict.fromkeys(capi.PAIR_STATS_FIELDS, 0), eq=n, eq_runs=1)


def test_stat_error_codes_follow_the_cigar_function():
    labels = [0, 1, 2, 3] * 5
    g = tip.path_graph(labels, [[0, 1, 2, 1, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])   # path 0 visits node 1 twice
    bad = tip.path_graph(labels, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    bad.path_nodes[4] = 1000
    codes = set()
    for graph, pairs in ((g, [(0, 1), (1, 0), (1, 9), (9, 1), (0, 0)]), (bad, [(1, 0), (0, 1), (0, 2), (1, 1)])):
        for a, b in pairs:
            want = tip.host_or_code(graph, a, b)
            got = stat_or_code(graph, a, b)
            assert got == (want if isinstance(want, int) else parse_cigar(want)), (a, b)
            if isinstance(want, int):
                codes.add(want)
    assert codes == {-1, -7}   # CL_ERR_INVALID_ARGUMENT, CL_ERR_CYCLIC_GRAPH


def formula(eq, x, ins, dele):
    """include/centrolign_amd.h, cl_alignment_distances"""
    den = 2 * eq + 2 * x + ins + dele
    if den == 0 or 2 * eq == den:
        return 0.0
    return 1.0 - float(2 * eq) / float(den)


def bits(v):
    return struct.pack("<d", float(v))


def test_alignment_distances_restated_bit_for_bit():
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_24x7k.gfa.gz"), "rb").read()))[0]
    n = len(g.path_off) - 1
    pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
    stats = np.array([[capi.induced_pairwise_stat(g, a, b)[k] for k in capi.PAIR_STATS_FIELDS] for a, b in pairs], np.uint64)
    rng = np.random.default_rng(12)
    rows = [stats, rng.integers(0, 1 << 40, (n * (n - 1) // 2, 8)).astype(np.uint64)]
    rows.append(rows[1].copy())
    rows[2][::3, 1:4] = 0          # identical pairs: 2 eq == den
    rows[2][1::3, 0:4] = 0         # two empty paths: den == 0
    for st in rows:
        d = capi.alignment_distances(st, n)
        assert d.shape == (n, n) and np.array_equal(d, d.T) and not d.diagonal().any()
        for k, (a, b) in enumerate(pairs):
            eq, x, ins, dele = (int(v) for v in st[k, :4])
            assert bits(d[a, b]) == bits(formula(eq, x, ins, dele)), (a, b)
    assert (capi.alignment_distances(stats, n)[np.triu_indices(n, 1)] > 0).all()


def test_alignment_distance_of_identical_paths_is_plus_zero():
    g = tip.path_graph([0, 1, 2, 3], [[0, 1, 2, 3], [0, 1, 2, 3]])
    st = capi.induced_pairwise_stat(g, 0, 1)
    assert st["eq"] == 4 and st["eq_runs"] == 1
    d = capi.alignment_distances([[st[k] for k in capi.PAIR_STATS_FIELDS]], 2)
    assert all(bits(v) == bits(0.0) for v in d.ravel())


def test_alignment_distances_needs_two_sequences():
    for n in (0, 1):
        with pytest.raises(capi.ClError) as e:
            capi.alignment_distances(np.zeros((0, 8), np.uint64), n)
        assert e.value.code == -1


# ---------------------------------------------------------------- the command line ----------------------------------------------------------
def run(args, cwd, timeout=60):
    r = subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    assert r.returncode >= 0, "killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace"))
    return r


def refused(r):
    lines = r.stderr.decode().splitlines()
    return r.returncode == 1 and r.stdout == b"" and len(lines) == 1 and lines[0].startswith("error: ")


def test_cli_refuses_before_reading_anything(tmp_path):
    """none of these names an input that exists: a refusal that came after reading the FASTA would be a different message"""
    existing = tmp_path / "stats.tsv"
    existing.write_text("kept\n")
    cases = [
        ["--refine-tree", "2", "-R", "-S", "sp", "missing.fa"],
        ["--refine-tree", "0", "missing.fa"],
        ["--refine-tree", "-3", "missing.fa"],
        ["--refine-tree", "1.5", "missing.fa"],
        ["--refine-tree", "two", "missing.fa"],
        ["--pair-stats", existing, "missing.fa"],
        ["--tree-out", "t.nwk", "missing.fa"],
    ]
    for args in cases:
        r = run(args, tmp_path)
        assert refused(r), (args, r.stderr)
        assert "missing.fa" not in r.stderr.decode(), args
        assert sorted(os.listdir(tmp_path)) == ["stats.tsv"], args
    assert existing.read_text() == "kept\n"
    assert run(["--tree-out", "t.nwk", "missing.fa"], tmp_path).stderr == b"error: --tree-out needs --infer-tree\n"
    # --tree-out is accepted with --refine-tree: the run gets as far as the missing FASTA
    r = run(["-v", "0", "--refine-tree", "2", "--tree-out", "t.nwk", "missing.fa"], tmp_path)
    assert refused(r) and "missing.fa" in r.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == ["stats.tsv"]


def test_cli_new_options_are_not_parameters(tmp_path):
    base = run(["-G"], tmp_path)
    got = run(["--pair-stats", "ps.tsv", "--dist-out", "d.txt", "--refine-tree", "3", "--tree-out", "t.nwk", "-G"], tmp_path)
    assert base.returncode == got.returncode == 0 and got.stdout == base.stdout and got.stderr == b""
    assert os.listdir(tmp_path) == []
    h = run(["-h"], tmp_path)
    assert h.returncode == 0
    for opt in ("--pair-stats FILE", "--dist-out FILE", "--refine-tree INT", "--tree-out FILE"):
        assert opt in h.stderr.decode(), opt


def test_msa_params_mirror_ends_with_pair_stats_path():
    """cl_msa_params grew by one field at its end: MsaParamsFull mirrors all of it, and a plain MsaParams (the fields before it) has room for
    what the library writes behind them"""
    import ctypes as C
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "centrolign_amd.h")).read()
    body = hdr[hdr.index("typedef struct cl_msa_params {"):hdr.index("} cl_msa_params;")]
    assert re.findall(r"^    (?:const char\*|const int\*|int|uint64_t|cl_\w+)\s+(\w+);", body, re.M)[-2:] == ["force_gfa_output", "pair_stats_path"]
    assert capi.MsaParamsFull.pair_stats_path.offset == C.sizeof(capi.MsaParams) and C.sizeof(capi.MsaParamsFull) == capi.MSA_PARAMS_BYTES
    full = capi.MsaParamsFull()
    full.pair_stats_path = b"set"
    lib.cl_msa_params_default(C.byref(full))
    assert full.pair_stats_path is None and full.force_gfa_output == 0 and full.max_tandem_duplication_search_rounds == 3
    old = capi.MsaParams()
    lib.cl_msa_params_default(C.byref(old))
    view = capi.MsaParamsFull.from_buffer(old)
    assert view.pair_stats_path is None and view.max_tandem_duplication_search_rounds == 3
    assert capi.Config().msa_params().subalignments_path is None


def test_cli_dist_out_refuses_to_overwrite_its_working_file(tmp_path):
    """--dist-out without --pair-stats passes the rows through FILE.pair-stats.tmp: a file of that name is not overwritten"""
    (tmp_path / "d.txt.pair-stats.tmp").write_text("kept\n")
    r = run(["--dist-out", "d.txt", "missing.fa"], tmp_path)
    assert refused(r) and "missing.fa" not in r.stderr.decode()
    assert os.listdir(tmp_path) == ["d.txt.pair-stats.tmp"] and (tmp_path / "d.txt.pair-stats.tmp").read_text() == "kept\n"
    # with --pair-stats no working file is needed
    r = run(["-v", "0", "--dist-out", "d.txt", "--pair-stats", "ps.tsv", "missing.fa"], tmp_path)
    assert refused(r) and "missing.fa" in r.stderr.decode()
    # two names that the rows could not tell apart are refused once the FASTA is read, before a device is opened
    (tmp_path / "in.fa").write_text(">a/b\nACGT\n>a_b\nACGA\n")
    r = run(["-v", "0", "--dist-out", "e.txt", "in.fa"], tmp_path)
    assert refused(r) and "apart" in r.stderr.decode() and not (tmp_path / "e.txt").exists()
