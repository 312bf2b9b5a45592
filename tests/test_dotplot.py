"""Windowed k-mer identity maps (cl_kmer_dotplot_host, cl_dotplot_tsv, the CLI's --dotplot options), without a GPU: the host definition against a
numpy restatement (np.unique per window, np.intersect1d per pair, Python integers for the threshold, math.pow for the identity), the window
edges, every refused argument, the ABI, and every refusal of the command line, which comes before a device is opened.  tests/test_gpu_dotplot.py
holds the device path against the same restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi
from tests.test_gpu_tree_infer import messy_sequences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _i
TSV_HEADER = "sample1\tstart1\tend1\tsample2\tstart2\tend2\tshared\tdistinct1\tdistinct2\tidentity\n"


def window_sets(seqs, k, W):
    """win_off [n + 1] and, per global window, the ascending distinct k-mer codes of the k-mers whose first base stands in it"""
    win_off, sets = [0], []
    for s in seqs:
        raw = s.encode() if isinstance(s, str) else bytes(s)
        L = len(raw)
        n_win = (L + W - 1) // W
        win_off.append(win_off[-1] + n_win)
        codes = CODE[np.frombuffer(raw, np.uint8)].astype(np.uint64)
        if L >= k:
            bad = np.concatenate([[0], np.cumsum(codes > 3)])
            starts = np.arange(L - k + 1)
            ok = bad[starts + k] == bad[starts]
            kmer = np.zeros(L - k + 1, np.uint64)
            for j in range(k):
                kmer = (kmer << np.uint64(2)) | (codes[j:j + L - k + 1] & np.uint64(3))
            starts, kmer = starts[ok], kmer[ok]
        else:
            starts, kmer = np.zeros(0, np.int64), np.zeros(0, np.uint64)
        for w in range(n_win):
            sets.append(np.unique(kmer[(starts >= w * W) & (starts < (w + 1) * W)]))
    return np.array(win_off, np.uint64), sets


def threshold_q(min_identity, k):
    return int(math.ceil(math.ldexp(math.pow(min_identity / 100.0, k), 32)))


def restated(seqs, k, W, min_identity, pairs=0):
    """the dict of capi.kmer_dotplot_host, restated; "considered" counts the pairs a <= b with two non-empty sides"""
    win_off, sets = window_sets(seqs, k, W)
    G = len(sets)
    distinct = np.array([len(x) for x in sets], np.uint32)
    q = threshold_q(min_identity, k)
    rows, considered = [], 0
    for s in range(len(seqs)):
        for a in range(int(win_off[s]), int(win_off[s + 1])):
            if not len(sets[a]):
                continue
            for b in range(a, int(win_off[s + 1]) if pairs == 1 else G):
                if not len(sets[b]):
                    continue
                considered += 1
                shared = len(np.intersect1d(sets[a], sets[b], assume_unique=True))
                denom = int(min(distinct[a], distinct[b]))
                if shared >= 1 and shared * 2 ** 32 >= q * denom:
                    rows.append((a, b, shared, denom))
    entries = np.array(rows, dtype=capi.DOTPLOT_ENTRY) if rows else np.zeros(0, capi.DOTPLOT_ENTRY)
    identity = np.array([100.0 * math.pow(float(r[2]) / float(r[3]), 1.0 / k) for r in rows], np.float64)
    return {"n_seq": len(seqs), "n_windows": G, "k": k, "window": W, "threshold_q": q, "win_off": win_off, "distinct": distinct, "entries": entries,
            "identity": identity, "considered": considered}


def same_plot(got, want):
    for key in ("n_seq", "n_windows", "k", "window", "threshold_q"):
        assert got[key] == want[key], key
    assert np.array_equal(got["win_off"], want["win_off"])
    assert np.array_equal(got["distinct"], want["distinct"])
    assert got["entries"].dtype.itemsize == 16 and got["entries"].tobytes() == want["entries"].tobytes()
    assert np.array_equal(got["identity"].view(np.uint64), want["identity"].view(np.uint64))


def tsv_rows(plot, names, seqs):
    """the rows of cl_dotplot_tsv from a plot dict"""
    off = [int(x) for x in plot["win_off"]]
    W = plot["window"]
    out = [TSV_HEADER]
    for e, ident in zip(plot["entries"], plot["identity"]):
        cols = []
        for g in (int(e["a"]), int(e["b"])):
            s = max(i for i in range(len(seqs)) if off[i] <= g)
            start = (g - off[s]) * W
            cols += [names[s], str(start), str(min(start + W, len(seqs[s])))]
        cols += [str(int(e["shared"])), str(int(plot["distinct"][e["a"]])), str(int(plot["distinct"][e["b"]])), "%.9g" % ident]
        out.append("\t".join(cols) + "\n")
    return "".join(out).encode()


# ---------------------------------------------------------------- the definition --------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 11, 21, 31])
@pytest.mark.parametrize("W", ["k", 64, 257])
def test_host_dotplot_of_messy_sequences(k, W):
    """an empty sequence, sequences shorter than k, runs of N, lower case and ambiguity codes; all pairs and pairs of one sequence.  With windows
    of k bases the whole input would have tens of thousands of windows and 10^8 pairs to restate: every sequence is cut to its first bases there
    (the restatement is kept near 400 windows)"""
    seqs = messy_sequences(k)
    if W == "k":
        W = k
        seqs = [s[:max(40, 4 * k)] for s in seqs]
    names = ["s%d" % i for i in range(len(seqs))]
    for pairs in (0, 1):
        want = restated(seqs, k, W, 86.0, pairs)
        got = capi.kmer_dotplot_host(seqs, k=k, window=W, pairs=pairs, min_identity=86.0, names=names)
        same_plot(got, want)
        assert got["tsv"] == tsv_rows(want, names, seqs)
        assert 0 < len(want["entries"])
    assert want["n_windows"] <= 700


def test_threshold():
    seqs = messy_sequences(3)[5:9]
    k, W = 7, 300
    everything = restated(seqs, k, W, 0.0)
    assert everything["threshold_q"] == 0 and len(everything["entries"]) > 50
    same_plot(capi.kmer_dotplot_host(seqs, k=k, window=W, min_identity=0.0), everything)
    full = capi.kmer_dotplot_host(seqs, k=k, window=W, min_identity=100.0)
    assert full["threshold_q"] == 2 ** 32
    keep = everything["entries"]["shared"] == everything["entries"]["denom"]
    assert full["entries"].tobytes() == everything["entries"][keep].tobytes() and 0 < keep.sum() < len(keep)
    for mi in (35.0, 50.0, 72.5):
        got = capi.kmer_dotplot_host(seqs, k=k, window=W, min_identity=mi)
        q = threshold_q(mi, k)
        keep = np.array([int(e["shared"]) * 2 ** 32 >= q * int(e["denom"]) for e in everything["entries"]])
        assert got["threshold_q"] == q
        assert got["entries"].tobytes() == everything["entries"][keep].tobytes()
    kept = [len(capi.kmer_dotplot_host(seqs, k=k, window=W, min_identity=mi)["entries"]) for mi in (0.0, 35.0, 50.0, 72.5, 100.0)]
    assert kept == sorted(kept, reverse=True) and kept[0] > kept[2] > kept[-1], kept


def test_defaults():
    lib = capi.load_library()
    p = capi.DotplotParams()
    lib.cl_dotplot_params_default.argtypes = [C.POINTER(capi.DotplotParams)]
    lib.cl_dotplot_params_default.restype = None
    lib.cl_dotplot_params_default(C.byref(p))
    assert (p.k, p.window, p.pairs, p.min_identity, p.tile_windows) == (21, 2000, 0, 86.0, 0)
    got = capi.kmer_dotplot_host(["ACGT" * 1200])
    assert (got["k"], got["window"], got["n_windows"], got["threshold_q"]) == (21, 2000, 3, threshold_q(86.0, 21))


def test_window_edges():
    k, W = 4, 16
    rng = np.random.default_rng(5)
    body = "".join("ACGT"[x] for x in rng.integers(0, 4, 3 * W + 1))
    exact, longer, shorter = body[:3 * W], body[:3 * W + 1], body[:3 * W - 1]
    got = capi.kmer_dotplot_host([exact, longer, shorter], k=k, window=W, min_identity=0.0)
    same_plot(got, restated([exact, longer, shorter], k, W, 0.0))
    assert got["win_off"].tolist() == [0, 3, 7, 10]   # a multiple of W: 3 windows; one base more: a fourth; one base less: still 3
    assert got["distinct"][6] == 0                    # the fourth window of `longer` holds one base, which starts no k-mer
    # a k-mer that starts in the last base of a window belongs to that window: CGTA starts at position 15 and occurs nowhere else
    marked = "A" * 15 + "CGTA" + "A" * 13
    one = capi.kmer_dotplot_host([marked], k=k, window=W, min_identity=0.0)
    same_plot(one, restated([marked], k, W, 0.0))
    assert one["distinct"].tolist() == [5, 3]   # AAAA AAAC AACG ACGT CGTA | GTAA TAAA AAAA
    assert [tuple(e) for e in one["entries"]] == [(0, 0, 5, 5), (0, 1, 1, 3), (1, 1, 3, 3)]
    # the last k - 1 positions of a sequence start no k-mer, and the next sequence's first window shares nothing with them: read as one text,
    # position 13 of the first sequence would start CGTC, the first k-mer of the second
    first, second = "A" * 13 + "CGT", "CGTC" + "C" * 12
    two = capi.kmer_dotplot_host([first, second], k=k, window=W, min_identity=0.0)
    same_plot(two, restated([first, second], k, W, 0.0))
    assert two["distinct"].tolist() == [4, 4]   # AAAA AAAC AACG ACGT | CGTC GTCC TCCC CCCC
    assert [tuple(e) for e in two["entries"]] == [(0, 0, 4, 4), (1, 1, 4, 4)]


def test_invalid_arguments():
    ok = dict(k=5, window=64, pairs=0, min_identity=86.0)
    seqs = ["ACGTACGTACGT"]
    capi.kmer_dotplot_host(seqs, **ok)
    bad = [("k", dict(k=0)), ("k", dict(k=32)), ("k", dict(k=-1)), ("window", dict(window=4)), ("window", dict(window=2 ** 20 + 1)),
           ("min_identity", dict(min_identity=-0.5)), ("min_identity", dict(min_identity=100.5)), ("min_identity", dict(min_identity=float("nan"))),
           ("min_identity", dict(min_identity=float("inf"))), ("pairs", dict(pairs=2)), ("tile_windows", dict(tile_windows=65))]
    for word, change in bad:
        with pytest.raises(capi.ClError) as e:
            capi.kmer_dotplot_host(seqs, **dict(ok, **change))
        assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    with pytest.raises(capi.ClError) as e:
        capi.kmer_dotplot_host([], **ok)
    assert e.value.code == -1
    capi.kmer_dotplot_host(seqs, k=5, window=2 ** 20)
    capi.kmer_dotplot_host(seqs, k=12, window=12)


def test_too_much_text_is_refused():
    """the lengths are checked before a base is read: 2^30 bases in all, from a buffer that is far shorter"""
    lib = capi.load_library()
    lib.cl_kmer_dotplot_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.DotplotParams), C.POINTER(capi.DotplotC)]
    lib.cl_dotplot_params_default.argtypes = [C.POINTER(capi.DotplotParams)]
    lib.cl_dotplot_params_default.restype = None
    p = capi.DotplotParams()
    lib.cl_dotplot_params_default(C.byref(p))
    bufs = (C.c_char_p * 2)(b"ACGT", b"ACGT")
    out = capi.DotplotC()
    for lens in ([2 ** 29, 2 ** 29], [2 ** 30, 0], [2 ** 64 - 1, 2]):
        arr = np.array(lens, np.uint64)
        assert lib.cl_kmer_dotplot_host(bufs, arr.ctypes.data, 2, C.byref(p), C.byref(out)) == -1
        assert b"lengths" in lib.cl_last_error(None)
    p.window, p.k = 1, 1   # 2^32 windows cannot be reached below 2^30 bases: the text limit comes first
    arr = np.array([2 ** 30 - 1, 1], np.uint64)
    assert lib.cl_kmer_dotplot_host(bufs, arr.ctypes.data, 2, C.byref(p), C.byref(out)) == -1


def test_abi():
    lib = capi.load_library()
    new = ["cl_dotplot_params_default", "cl_kmer_dotplot_host", "cl_kmer_dotplot_compute", "cl_dotplot_tsv", "cl_dotplot_free"]
    for sym in new:
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert capi.ABI_VERSION == 22 == lib.cl_abi_version()
    assert C.sizeof(capi.DotplotEntry) == 16 == capi.DOTPLOT_ENTRY.itemsize
    # the header's layouts by hand (LP64): {int, u32, int, pad, double, u32, pad}, 4 x u32, {2 x u64, int, u32, u64, 2 pointers, u64, 2 pointers, 2 floats}
    assert [C.sizeof(capi.DotplotParams), C.sizeof(capi.DotplotEntry), C.sizeof(capi.DotplotC)] == [32, 16, 80]
    # and the C compiler's own sizes from the header itself, where there is a compiler
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is not None:
        src = '#include <stdio.h>\n#include "centrolign_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(cl_dotplot_params), sizeof(cl_dotplot_entry), sizeof(cl_dotplot)); return 0; }\n'
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "s.c"), "w") as f:
                f.write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
            sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()]
        assert sizes == [32, 16, 80]


# ---------------------------------------------------------------- the command line ------------------------------------------------------------
def run_cli(args, **kw):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=60, **kw)


@pytest.fixture()
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGAACGTACGTACGTACGTACGT\n>c\nACGTACGAACGTACGTACGGACGTACGT\n")
    return p


def refusals(tmp_path, fasta):
    out, old, other = tmp_path / "plot.tsv", tmp_path / "old.tsv", tmp_path / "other.tsv"
    old.write_text("keep me\n")
    d = ["--dotplot", out]
    return {
        "an existing file": ["--dotplot", old, fasta],
        "the file of --pair-stats": d + ["--pair-stats", out, fasta],
        "the file of --tree-out": d + ["--infer-tree", "--tree-out", out, fasta],
        "the file of --msa-out": d + ["--msa-out", out, fasta],
        "the file of -s": d + ["-s", out, fasta],
        "k 0": d + ["--dotplot-k", 0, fasta],
        "k 32": d + ["--dotplot-k", 32, fasta],
        "k not a number": d + ["--dotplot-k", "x", fasta],
        "window below k": d + ["--dotplot-k", 11, "--dotplot-window", 10, fasta],
        "window above 2^20": d + ["--dotplot-window", 2 ** 20 + 1, fasta],
        "identity below 0": d + ["--dotplot-min-identity", "-1", fasta],
        "identity above 100": d + ["--dotplot-min-identity", "100.01", fasta],
        "identity nan": d + ["--dotplot-min-identity", "nan", fasta],
        "identity not a number": d + ["--dotplot-min-identity", "high", fasta],
        "pairs word": d + ["--dotplot-pairs", "cross", fasta],
        "--dotplot-k alone": ["--dotplot-k", 11, fasta],
        "--dotplot-window alone": ["--dotplot-window", 100, fasta],
        "--dotplot-min-identity alone": ["--dotplot-min-identity", 50, fasta],
        "--dotplot-pairs alone": ["--dotplot-pairs", "self", fasta],
        "--dotplot-only alone": ["--dotplot-only", fasta],
        "with --graph": d + ["--graph", other, "--compare-to", other, "--pair-agreement", tmp_path / "agree.tsv"],
        "only with -T": d + ["--dotplot-only", "-T", other, fasta],
        "only with --infer-tree": d + ["--dotplot-only", "--infer-tree", fasta],
        "only with --pair-stats": d + ["--dotplot-only", "--pair-stats", other, fasta],
        "only with -c": d + ["--dotplot-only", "-c", fasta],
        "only with -t": d + ["--dotplot-only", "-t", 2, fasta],
        "only with --force-gfa-output": d + ["--dotplot-only", "--force-gfa-output", fasta],
        "only with -C": d + ["--dotplot-only", "-C", other, fasta],
    }


def test_cli_refusals(tmp_path, fasta):
    """each is one "error:" line and status 1 with nothing on standard output, before the FASTA is read or a device opened: the input file of
    half the cases does not even exist, and CL_NO_DEVICE-style failures would read differently"""
    cases = refusals(tmp_path, fasta)
    assert len(cases) >= 25
    for name, args in cases.items():
        r = run_cli(args)
        err = r.stderr.decode().splitlines()
        assert r.returncode == 1 and r.stdout == b"", (name, r.returncode, r.stderr)
        assert len(err) == 1 and err[0].startswith("error: ") and "GPU" not in err[0], (name, err)
        assert not (tmp_path / "plot.tsv").exists(), name
        assert (tmp_path / "old.tsv").read_text() == "keep me\n", name
    # the same refusals without a FASTA that could be read: they come first
    r = run_cli(["--dotplot", tmp_path / "plot.tsv", "--dotplot-k", 40, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"--dotplot-k" in r.stderr and b"missing.fa" not in r.stderr


def test_cli_generate_config_and_help(tmp_path):
    plain = run_cli(["-G"])
    with_options = run_cli(["-G", "--dotplot", tmp_path / "plot.tsv", "--dotplot-k", 15, "--dotplot-window", 500, "--dotplot-min-identity", 90,
                            "--dotplot-pairs", "self"])
    assert plain.returncode == 0 and with_options.returncode == 0 and plain.stdout == with_options.stdout and plain.stdout
    assert not (tmp_path / "plot.tsv").exists()
    text = run_cli(["-h"]).stderr.decode()
    for opt in ("--dotplot FILE", "--dotplot-k INT", "--dotplot-window INT", "--dotplot-min-identity FLOAT", "--dotplot-pairs", "--dotplot-only"):
        assert opt in text, opt
