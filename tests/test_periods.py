"""Repeat period spectra (cl_period_spectrum_host, cl_period_peaks_host, the two TSV writers, the CLI's --periods options), without a GPU: the host
definition against a numpy restatement (a stable argsort of the keys per sequence, np.add.at for the rows, the peak rule in plain Python), an exact
tandem array on both sides of the d = max_period edge, higher-order-repeat arrays, the peak rule on hand-made rows, the text, every refused
argument, the ABI, and every refusal of the command line, which comes before a device is opened.  tests/test_gpu_periods.py holds the device path
against the same restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests.test_gpu_tree_infer import messy_sequences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    CODE[ord(_c)] = CODE[ord(_c.lower())] = _i
DEFAULTS = dict(n_peaks=3, peak_radius=1, min_period=1, min_count=2)
COUNTERS = ("kmers", "links", "far", "last")
TSV_HEADER = "sample\tstart\tend\tkmers\tlinks\tfar\trank\tperiod\tcount\tshare\n"
HIST_HEADER = "sample\tstart\tend\tperiod\tcount\n"


def occurrences(seq, k):
    """(start positions, k-mer codes) of the k-mers of one sequence, in text order"""
    raw = seq.encode() if isinstance(seq, str) else bytes(seq)
    L = len(raw)
    if L < k:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    codes = CODE[np.frombuffer(raw, np.uint8)].astype(np.uint64)
    bad = np.concatenate([[0], np.cumsum(codes > 3)])
    starts = np.arange(L - k + 1)
    ok = bad[starts + k] == bad[starts]
    kmer = np.zeros(L - k + 1, np.uint64)
    for j in range(k):
        kmer = (kmer << np.uint64(2)) | (codes[j:j + L - k + 1] & np.uint64(3))
    return starts[ok], kmer[ok]


def peaks_of(h, D, n_peaks, peak_radius, min_period, min_count):
    """the peak rule, bin by bin"""
    found = []
    for d in np.nonzero(h[:D + 1] >= min_count)[0]:
        d = int(d)
        if d < max(min_period, 1):
            continue
        left, right = h[max(1, d - peak_radius):d], h[d + 1:min(D, d + peak_radius) + 1]
        if (h[d] > left).all() and (h[d] >= right).all():
            found.append((-int(h[d]), d))
    found.sort()
    out = np.zeros(n_peaks, capi.PERIOD_PEAK)
    for i, (c, d) in enumerate(found[:n_peaks]):
        out[i] = (d, -c)
    return out


def restated(seqs, k, W, D, n_peaks=3, peak_radius=1, min_period=1, min_count=2):
    """the dict of capi.period_spectrum_host, restated"""
    n = len(seqs)
    win_off = np.concatenate([[0], np.cumsum([(len(s) + W - 1) // W for s in seqs])]).astype(np.uint64)
    G = int(win_off[-1])
    R = G + n
    hist = np.zeros((R, D + 1), np.uint32)
    cnt = {name: np.zeros(R, np.uint32) for name in COUNTERS}
    for s, seq in enumerate(seqs):
        pos, key = occurrences(seq, k)
        order = np.argsort(key, kind="stable")
        pos, key = pos[order], key[order]
        g = int(win_off[s]) + pos // W
        has_next = np.zeros(len(pos), bool)
        has_next[:-1] = key[1:] == key[:-1]
        d = np.zeros(len(pos), np.int64)
        d[:-1] = pos[1:] - pos[:-1]
        link, far = has_next & (d <= D), has_next & (d > D)
        assert (d[has_next] >= 1).all()
        np.add.at(hist, (g[link], d[link]), 1)
        np.add.at(hist, (g[far], 0), 1)
        np.add.at(cnt["kmers"], g, 1)
        np.add.at(cnt["links"], g[link], 1)
        np.add.at(cnt["far"], g[far], 1)
        np.add.at(cnt["last"], g[~has_next], 1)
        mine = slice(int(win_off[s]), int(win_off[s + 1]))
        hist[G + s] = hist[mine].sum(axis=0, dtype=np.uint32)
        for name in COUNTERS:
            cnt[name][G + s] = cnt[name][mine].sum()
    peaks = np.stack([peaks_of(hist[r], D, n_peaks, peak_radius, min_period, min_count) for r in range(R)])
    out = {"n_seq": n, "n_windows": G, "n_rows": R, "k": k, "window": W, "max_period": D, "n_peaks": n_peaks, "win_off": win_off, "hist": hist, "peaks": peaks}
    out.update(cnt)
    return out


def same_spectrum(got, want, hist=True):
    for key in ("n_seq", "n_windows", "n_rows", "k", "window", "max_period", "n_peaks"):
        assert got[key] == want[key], key
    assert np.array_equal(got["win_off"], want["win_off"])
    for name in COUNTERS:
        assert got[name].dtype == np.uint32 and np.array_equal(got[name], want[name]), name
    assert got["peaks"].dtype.itemsize == 8 and got["peaks"].shape == want["peaks"].shape and got["peaks"].tobytes() == want["peaks"].tobytes()
    if hist:
        assert got["hist"].shape == want["hist"].shape and got["hist"].tobytes() == want["hist"].tobytes()
    else:
        assert got["hist"] is None


def identities(sp):
    """kmers = links + far + last, links = the bins 1..D, far = bin 0, and row G + s = the sum of the rows of s"""
    h = sp["hist"].astype(np.int64)
    assert np.array_equal(sp["kmers"], sp["links"] + sp["far"] + sp["last"])
    assert np.array_equal(sp["links"], h[:, 1:].sum(axis=1)) and np.array_equal(sp["far"], h[:, 0])
    G, off = sp["n_windows"], sp["win_off"]
    for s in range(sp["n_seq"]):
        mine = slice(int(off[s]), int(off[s + 1]))
        assert np.array_equal(h[G + s], h[mine].sum(axis=0))
        for name in COUNTERS:
            assert sp[name][G + s] == sp[name][mine].sum()


def rows_in_order(sp, lengths, scope):
    """(sequence, row, start, end) as both TSV writers go through the rows"""
    G, off, W = sp["n_windows"], [int(x) for x in sp["win_off"]], sp["window"]
    for s in range(sp["n_seq"]):
        if scope != 2:
            yield s, G + s, 0, lengths[s]
        if scope != 1:
            for g in range(off[s], off[s + 1]):
                start = (g - off[s]) * W
                yield s, g, start, min(start + W, lengths[s])


def tsv_rows(sp, names, lengths, scope=0):
    out = [TSV_HEADER]
    for s, r, start, end in rows_in_order(sp, lengths, scope):
        lead = [names[s], str(start), str(end), str(sp["kmers"][r]), str(sp["links"][r]), str(sp["far"][r])]
        peaks = [p for p in sp["peaks"][r] if p["count"]]
        if not peaks:
            out.append("\t".join(lead + ["0", "0", "0", "0"]) + "\n")
        for i, p in enumerate(peaks):
            out.append("\t".join(lead + [str(i + 1), str(p["period"]), str(p["count"]), "%.9g" % (float(p["count"]) / float(sp["links"][r]))]) + "\n")
    return "".join(out).encode()


def hist_rows(sp, names, lengths, scope=0):
    out = [HIST_HEADER]
    for s, r, start, end in rows_in_order(sp, lengths, scope):
        h = sp["hist"][r]
        for d in np.nonzero(h[1:])[0] + 1:
            out.append("%s\t%d\t%d\t%d\t%d\n" % (names[s], start, end, d, h[d]))
    return "".join(out).encode()


# ---------------------------------------------------------------- the definition --------------------------------------------------------------
def messy_case(k, W):
    """the inputs of the messy sweep: windows of one base only on the sequences cut to 200 bases, which keeps R * (D + 1) small"""
    seqs = messy_sequences(k)
    return [s[:200] for s in seqs] if W == 1 else seqs


@pytest.mark.parametrize("k", [1, 4, 8, 21, 31])
@pytest.mark.parametrize("W", [1, 64, 257, 2 ** 20])
def test_host_spectrum_of_messy_sequences(k, W):
    """an empty sequence, sequences shorter than k, runs of N, lower case and ambiguity codes"""
    seqs = messy_case(k, W)
    for D in (1, 50, 4096):
        want = restated(seqs, k, W, D)
        got = capi.period_spectrum_host(seqs, k=k, window=W, max_period=D)
        same_spectrum(got, want)
        identities(got)
        assert (got["kmers"][:got["n_windows"]] == 0).any() and got["kmers"].sum() > 0
        assert got["links_ms"] == 0 and got["hist_ms"] == 0


def cyclic_unit(seed=3, length=37, k=8):
    rng = np.random.default_rng(seed)
    while True:
        unit = "".join("ACGT"[x] for x in rng.integers(0, 4, length))
        twice = unit + unit
        if len({twice[i:i + k] for i in range(length)}) == length:
            return unit


def test_exact_tandem_array():
    unit = cyclic_unit()
    assert len(unit) == 37 and len({(unit + unit)[i:i + 8] for i in range(37)}) == 37   # its 8-mers, read cyclically, are distinct
    seq = unit * 100
    at = capi.period_spectrum_host([seq], k=8, window=2 ** 20, max_period=37)
    same_spectrum(at, restated([seq], 8, 2 ** 20, 37))
    for r in (0, 1):   # the window and the sequence's total
        assert (at["kmers"][r], at["last"][r], at["links"][r], at["far"][r]) == (3693, 37, 3656, 0)
        assert at["hist"][r, 37] == 3656 and at["hist"][r].sum() == 3656
        assert at["peaks"][r].tolist() == [(37, 3656), (0, 0), (0, 0)]
    below = capi.period_spectrum_host([seq], k=8, window=2 ** 20, max_period=36)
    same_spectrum(below, restated([seq], 8, 2 ** 20, 36))
    for r in (0, 1):
        assert (below["kmers"][r], below["last"][r], below["links"][r], below["far"][r]) == (3693, 37, 0, 3656)
        assert below["hist"][r, 0] == 3656 and below["hist"][r].sum() == 3656
        assert below["peaks"][r].tolist() == [(0, 0)] * 3
    # the same sequence twice: the same rows twice, no link crosses a sequence boundary
    two = capi.period_spectrum_host([seq, seq], k=8, window=1000, max_period=37)
    same_spectrum(two, restated([seq, seq], 8, 1000, 37))
    assert two["n_windows"] == 8 and np.array_equal(two["hist"][0:4], two["hist"][4:8]) and np.array_equal(two["hist"][8], two["hist"][9])
    assert np.array_equal(two["hist"][8], at["hist"][1]) and two["last"][8] == two["last"][9] == 37
    for name in COUNTERS:
        assert np.array_equal(two[name][0:4], two[name][4:8])


@pytest.fixture(scope="module")
def hor():
    seqs = synth.hor_sequences(5, 6000, 3)
    assert [len(s) for s in seqs] == [5998, 10128, 5996]
    return seqs


def test_hor_arrays(hor):
    """the total of sequence 1: at k = 8 the top peak is the period of the higher-order repeat (12 monomers of about 171 bases), at k = 4 the monomer"""
    k8 = capi.period_spectrum_host(hor, k=8, window=2 ** 20, max_period=4096)
    same_spectrum(k8, restated(hor, 8, 2 ** 20, 4096))
    r = k8["n_windows"] + 1
    assert (k8["kmers"][r], k8["links"][r], k8["far"][r], k8["last"][r]) == (10121, 7516, 146, 2459)
    assert k8["peaks"][r].tolist() == [(2064, 3383), (2060, 696), (2066, 272)]
    assert abs(int(k8["peaks"][r][0]["period"]) - 2052) <= 20
    k4 = capi.period_spectrum_host(hor, k=4, window=2 ** 20, max_period=4096)
    same_spectrum(k4, restated(hor, 4, 2 ** 20, 4096))
    assert k4["peaks"][r].tolist()[:2] == [(173, 157), (168, 116)]
    assert abs(int(k4["peaks"][r][0]["period"]) - 171) <= 5
    for sp in (k8, k4):
        identities(sp)


# ---------------------------------------------------------------- the peak rule ---------------------------------------------------------------
def row(D, **bins):
    h = np.zeros(D + 1, np.uint32)
    for d, c in bins.items():
        h[int(d[1:])] = c
    return h


def peaks(h, **kw):
    got = capi.period_peaks_host(h, **kw)
    p = dict(DEFAULTS, **kw)
    assert got.tobytes() == peaks_of(np.asarray(h), len(h) - 1, p["n_peaks"], p["peak_radius"], p["min_period"], p["min_count"]).tobytes()
    return got.tolist()


def test_peak_rule_on_hand_made_rows():
    # a plateau: the leftmost bin wins
    assert peaks(row(100, b40=7, b41=7, b42=7)) == [(40, 7), (0, 0), (0, 0)]
    assert peaks(row(100, b40=7, b41=7, b42=7), peak_radius=5) == [(40, 7), (0, 0), (0, 0)]
    # equal counts: the smaller period first
    assert peaks(row(100, b90=5, b30=5, b60=9)) == [(60, 9), (30, 5), (90, 5)]
    # a jittered pair: two peaks at radius 1, one at radius 5
    jitter = row(4096, b2060=696, b2064=3383, b171=40)
    assert peaks(jitter) == [(2064, 3383), (2060, 696), (171, 40)]
    assert peaks(jitter, peak_radius=5) == [(2064, 3383), (171, 40), (0, 0)]
    assert peaks(jitter, peak_radius=3) == [(2064, 3383), (2060, 696), (171, 40)]   # 4 bins apart: outside a radius of 3
    # min_period and min_count each exclude a bin that would otherwise win
    assert peaks(row(300, b2=900, b171=50)) == [(2, 900), (171, 50), (0, 0)]
    assert peaks(row(300, b2=900, b171=50), min_period=3) == [(171, 50), (0, 0), (0, 0)]
    assert peaks(row(300, b2=900, b171=50), min_count=51) == [(2, 900), (0, 0), (0, 0)]
    assert peaks(row(300, b2=900, b171=50), min_count=901) == [(0, 0)] * 3
    assert peaks(row(300, b7=1)) == [(0, 0)] * 3 and peaks(row(300, b7=1), min_count=1) == [(7, 1), (0, 0), (0, 0)]
    assert peaks(row(300, b2=900), min_period=301) == [(0, 0)] * 3
    # fewer candidates than n_peaks: zero-filled slots; more: the best n_peaks
    assert peaks(row(50, b10=4), n_peaks=16) == [(10, 4)] + [(0, 0)] * 15
    assert peaks(row(50, b10=4, b20=6, b30=5), n_peaks=1) == [(20, 6)]
    # a peak at d = 1 and one at d = D: the bins beyond either end read as 0
    assert peaks(row(64, b1=3, b64=8)) == [(64, 8), (1, 3), (0, 0)]
    assert peaks(row(64, b1=3, b2=3, b63=8, b64=8), peak_radius=64) == [(63, 8), (0, 0), (0, 0)]
    assert peaks(row(1, b1=2)) == [(1, 2), (0, 0), (0, 0)]
    # bin 0 ("far") is large and ignored: it neither is a peak nor shadows bin 1
    assert peaks(row(64, b0=10 ** 6, b1=3, b30=2)) == [(1, 3), (30, 2), (0, 0)]
    # a descending slope has one peak, an ascending one too
    assert peaks(np.arange(20, 0, -1).astype(np.uint32), n_peaks=4) == [(1, 19), (0, 0), (0, 0), (0, 0)]
    assert peaks(np.arange(0, 20).astype(np.uint32), n_peaks=4) == [(19, 19), (0, 0), (0, 0), (0, 0)]


def test_peak_parameters_on_the_hor_case(hor):
    for kw in (dict(n_peaks=1), dict(n_peaks=16), dict(peak_radius=5), dict(peak_radius=64), dict(min_period=200), dict(min_count=1), dict(min_count=1000)):
        got = capi.period_spectrum_host(hor, k=8, window=2000, max_period=4096, **kw)
        same_spectrum(got, restated(hor, 8, 2000, 4096, **kw))


# ---------------------------------------------------------------- text and plumbing -----------------------------------------------------------
def test_defaults():
    lib = capi.load_library()
    p = capi.PeriodsParams()
    lib.cl_periods_params_default.argtypes = [C.POINTER(capi.PeriodsParams)]
    lib.cl_periods_params_default.restype = None
    lib.cl_periods_params_default(C.byref(p))
    assert (p.k, p.window, p.max_period, p.n_peaks, p.peak_radius, p.min_period, p.min_count, p.want_hist) == (8, 10000, 8000, 3, 1, 1, 2, 1)
    got = capi.period_spectrum_host(["ACGT" * 6000])
    assert (got["k"], got["window"], got["max_period"], got["n_peaks"], got["n_windows"], got["n_rows"]) == (8, 10000, 8000, 3, 3, 4)
    assert got["hist"].shape == (4, 8001) and got["peaks"].shape == (4, 3) and got["peaks"][3].tolist() == [(4, 23989), (0, 0), (0, 0)]


def test_tsv(hor):
    names = ["a_1", "b", "c"]
    lengths = [len(s) for s in hor]
    sp = capi.period_spectrum_host(hor, k=8, window=2000, max_period=4096)
    assert any(p["count"] == 0 for p in sp["peaks"][:, 0]) and any(p["count"] for p in sp["peaks"][:, 2])   # rows without a peak and full rows
    for scope, word in ((0, "both"), (1, "sequences"), (2, "windows")):
        want = tsv_rows(sp, names, lengths, scope)
        assert capi.periods_tsv(sp, names, lengths, scope) == want == capi.periods_tsv(sp, names, lengths, word)
        want_hist = hist_rows(sp, names, lengths, scope)
        assert capi.periods_hist_tsv(sp, names, lengths, scope) == want_hist == capi.periods_hist_tsv(sp, names, lengths, word)
        assert want.endswith(b"\n") and want_hist.endswith(b"\n")
    both, only_seq, only_win = (tsv_rows(sp, names, lengths, s).splitlines() for s in (0, 1, 2))
    assert len(both) - 1 == len(only_seq) - 1 + len(only_win) - 1 and len(only_seq) - 1 == 9
    assert both[1].split(b"\t")[:3] == [b"a_1", b"0", b"5998"] and both[4].split(b"\t")[:3] == [b"a_1", b"0", b"2000"]   # the total, then the windows
    assert any(line.startswith(b"a_1\t4000\t5998\t") for line in only_win) and not any(line.startswith(b"a_1\t4000\t6000\t") for line in only_win)   # the end is clipped
    # an empty sequence has a total row and no window; a sequence without a k-mer has zeros
    odd = ["", "ACGTACGTAC", "NNNN"]
    sp = capi.period_spectrum_host(odd, k=4, window=8, max_period=5)
    text = capi.periods_tsv(sp, ["e", "f", "g"], [0, 10, 4])
    assert text == tsv_rows(sp, ["e", "f", "g"], [0, 10, 4])
    assert text.splitlines()[1] == b"e\t0\t0\t0\t0\t0\t0\t0\t0\t0" and b"f\t0\t10\t7\t3\t0\t1\t4\t3\t1" in text.splitlines()
    # without the rows there is no histogram text, and the peak text is the same
    lean = capi.period_spectrum_host(hor, k=8, window=2000, max_period=4096, want_hist=0)
    full = capi.period_spectrum_host(hor, k=8, window=2000, max_period=4096)
    same_spectrum(lean, full, hist=False)
    assert capi.periods_tsv(lean, names, lengths) == capi.periods_tsv(full, names, lengths)
    with pytest.raises(capi.ClError) as e:
        capi.periods_hist_tsv(lean, names, lengths)
    assert e.value.code == -1 and "hist" in str(e.value)
    with pytest.raises(capi.ClError) as e:
        capi.periods_tsv(full, names, lengths, 3)
    assert e.value.code == -1 and "scope" in str(e.value)


def test_invalid_arguments():
    ok = dict(k=5, window=64, max_period=50)
    seqs = ["ACGTACGTACGT"]
    capi.period_spectrum_host(seqs, **ok)
    bad = [("k", dict(k=0)), ("k", dict(k=32)), ("k", dict(k=-1)), ("window", dict(window=0)), ("window", dict(window=2 ** 20 + 1)),
           ("max_period", dict(max_period=0)), ("max_period", dict(max_period=16384)), ("n_peaks", dict(n_peaks=0)), ("n_peaks", dict(n_peaks=17)),
           ("peak_radius", dict(peak_radius=0)), ("peak_radius", dict(peak_radius=65)), ("min_period", dict(min_period=0)), ("min_count", dict(min_count=0))]
    for word, change in bad:
        with pytest.raises(capi.ClError) as e:
            capi.period_spectrum_host(seqs, **dict(ok, **change))
        assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
        if word in ("n_peaks", "peak_radius", "min_period", "min_count"):
            with pytest.raises(capi.ClError) as e:
                capi.period_peaks_host(np.zeros(51, np.uint32), **change)
            assert e.value.code == -1 and word in str(e.value), (change, str(e.value))
    with pytest.raises(capi.ClError) as e:
        capi.period_spectrum_host([], **ok)
    assert e.value.code == -1 and "n" in str(e.value)
    # R * (D + 1) <= 2^28: 16 384 windows and one total of 16 384 bins are one row too many
    with pytest.raises(capi.ClError) as e:
        capi.period_spectrum_host(["A" * 16384], k=1, window=1, max_period=16383)
    assert e.value.code == -1 and "max_period" in str(e.value) and "window" in str(e.value)
    # the largest values of every argument are accepted
    capi.period_spectrum_host(seqs, k=31, window=2 ** 20, max_period=16383, n_peaks=16, peak_radius=64, min_period=2 ** 32 - 1, min_count=2 ** 32 - 1)
    capi.period_spectrum_host(seqs, k=1, window=1, max_period=1, n_peaks=1, peak_radius=1, min_period=1, min_count=1)


def test_too_much_text_is_refused():
    """the lengths are checked before a base is read: 2^30 bases in all, from a buffer that is far shorter"""
    lib = capi.load_library()
    lib.cl_period_spectrum_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.PeriodsParams), C.POINTER(capi.PeriodSpectrumC)]
    lib.cl_periods_params_default.argtypes = [C.POINTER(capi.PeriodsParams)]
    lib.cl_periods_params_default.restype = None
    p = capi.PeriodsParams()
    lib.cl_periods_params_default(C.byref(p))
    bufs = (C.c_char_p * 2)(b"ACGT", b"ACGT")
    out = capi.PeriodSpectrumC()
    for lens in ([2 ** 29, 2 ** 29], [2 ** 30, 0], [2 ** 64 - 1, 2]):
        arr = np.array(lens, np.uint64)
        assert lib.cl_period_spectrum_host(bufs, arr.ctypes.data, 2, C.byref(p), C.byref(out)) == -1
        assert b"lengths" in lib.cl_last_error(None)


def test_abi():
    lib = capi.load_library()
    new = ["cl_periods_params_default", "cl_period_spectrum_host", "cl_period_spectrum_compute", "cl_period_peaks_host", "cl_periods_tsv", "cl_periods_hist_tsv",
           "cl_period_spectrum_free"]
    for sym in new:
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(capi.PeriodPeak) == 8 == capi.PERIOD_PEAK.itemsize
    # the header's layouts by hand (LP64): 8 x 4 bytes, 2 x u32, {3 x u64, int, 3 x u32, 7 pointers, 2 floats}
    assert [C.sizeof(capi.PeriodsParams), C.sizeof(capi.PeriodPeak), C.sizeof(capi.PeriodSpectrumC)] == [32, 8, 104]
    # and the C compiler's own sizes from the header itself, where there is a compiler
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is not None:
        src = ('#include <stdio.h>\n#include "centrolign_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(cl_periods_params), sizeof(cl_period_peak), '
               'sizeof(cl_period_spectrum)); return 0; }\n')
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "s.c"), "w") as f:
                f.write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
            sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()]
        assert sizes == [32, 8, 104]


# ---------------------------------------------------------------- the command line ------------------------------------------------------------
def run_cli(args, **kw):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=60, **kw)


@pytest.fixture()
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGAACGTACGTACGTACGTACGT\n>c\nACGTACGAACGTACGTACGGACGTACGT\n")
    return p


NUMBERS = {"--periods-k": (31, 8), "--periods-window": (2 ** 20, 100), "--periods-max": (16383, 100), "--periods-peaks": (16, 2), "--periods-radius": (64, 2),
           "--periods-min-period": (None, 2), "--periods-min-count": (None, 2)}


def refusals(tmp_path, fasta):
    out, hist, old, other = tmp_path / "periods.tsv", tmp_path / "hist.tsv", tmp_path / "old.tsv", tmp_path / "other.tsv"
    old.write_text("keep me\n")
    d = ["--periods", out]
    cases = {
        "an existing file": ["--periods", old, fasta],
        "an existing histogram file": d + ["--periods-hist", old, fasta],
        "one file for both": d + ["--periods-hist", out, fasta],
        "the file of --pair-stats": d + ["--pair-stats", out, fasta],
        "the file of --tree-out": d + ["--infer-tree", "--tree-out", out, fasta],
        "the file of --msa-out": d + ["--msa-out", out, fasta],
        "the file of -s": d + ["-s", out, fasta],
        "the file of --dotplot": d + ["--dotplot", out, fasta],
        "the histogram in the file of --column-stats": d + ["--periods-hist", hist, "--column-stats", hist, fasta],
        "scope word": d + ["--periods-scope", "rows", fasta],
        "--periods-hist alone": ["--periods-hist", hist, fasta],
        "--periods-scope alone": ["--periods-scope", "both", fasta],
        "--periods-only alone": ["--periods-only", fasta],
        "with --graph": d + ["--graph", other, "--compare-to", other, "--pair-agreement", tmp_path / "agree.tsv"],
        "only with -T": d + ["--periods-only", "-T", other, fasta],
        "only with --infer-tree": d + ["--periods-only", "--infer-tree", fasta],
        "only with --pair-stats": d + ["--periods-only", "--pair-stats", other, fasta],
        "only with -c": d + ["--periods-only", "-c", fasta],
        "only with -t": d + ["--periods-only", "-t", 2, fasta],
        "only with --force-gfa-output": d + ["--periods-only", "--force-gfa-output", fasta],
        "only with -C": d + ["--periods-only", "-C", other, fasta],
        "only with --dotplot": d + ["--periods-only", "--dotplot", other, fasta],
        "--dotplot-only with --periods": ["--dotplot", other, "--dotplot-only"] + d + [fasta],
        "both -only options": ["--dotplot", other, "--dotplot-only"] + d + ["--periods-only", fasta],
    }
    for opt, (most, fine) in NUMBERS.items():
        cases[opt + " 0"] = d + [opt, 0, fasta]
        cases[opt + " not a number"] = d + [opt, "x", fasta]
        cases[opt + " negative"] = d + [opt, "-3", fasta]
        cases[opt + " a fraction"] = d + [opt, "2.5", fasta]
        cases[opt + " alone"] = [opt, fine, fasta]
        if most is not None:
            cases[opt + " above the limit"] = d + [opt, most + 1, fasta]
    return cases


def test_cli_refusals(tmp_path, fasta):
    """each is one "error:" line and status 1 with nothing on standard output, before the FASTA is read or a device opened"""
    cases = refusals(tmp_path, fasta)
    assert len(cases) >= 60
    for name, args in cases.items():
        r = run_cli(args)
        err = r.stderr.decode().splitlines()
        assert r.returncode == 1 and r.stdout == b"", (name, r.returncode, r.stderr)
        assert len(err) == 1 and err[0].startswith("error: ") and "GPU" not in err[0], (name, err)
        for made in ("periods.tsv", "hist.tsv", "other.tsv"):
            assert not (tmp_path / made).exists(), (name, made)
        assert (tmp_path / "old.tsv").read_text() == "keep me\n", name
    # the same refusals without a FASTA that could be read: they come first
    r = run_cli(["--periods", tmp_path / "periods.tsv", "--periods-max", 20000, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"--periods-max" in r.stderr and b"missing.fa" not in r.stderr
    # the largest values pass the option checks: the run then ends at the FASTA that is not there
    args = ["--periods", tmp_path / "periods.tsv", "--periods-hist", tmp_path / "hist.tsv", "--periods-only", "--periods-scope", "windows"]
    for opt, (most, fine) in NUMBERS.items():
        args += [opt, most if most is not None else 2 ** 32 - 1]
    r = run_cli(args + [tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"missing.fa" in r.stderr and not (tmp_path / "periods.tsv").exists()


def test_cli_generate_config_help_and_abbreviations(tmp_path):
    plain = run_cli(["-G"])
    with_options = run_cli(["-G", "--periods", tmp_path / "periods.tsv", "--periods-hist", tmp_path / "hist.tsv", "--periods-k", 6, "--periods-window", 500,
                            "--periods-max", 300, "--periods-peaks", 5, "--periods-radius", 2, "--periods-min-period", 3, "--periods-min-count", 4,
                            "--periods-scope", "windows"])
    assert plain.returncode == 0 and with_options.returncode == 0 and plain.stdout == with_options.stdout and plain.stdout
    assert not (tmp_path / "periods.tsv").exists() and not (tmp_path / "hist.tsv").exists()
    text = run_cli(["-h"]).stderr.decode()
    for opt in ("--periods FILE", "--periods-hist FILE", "--periods-k INT", "--periods-window INT", "--periods-max INT", "--periods-peaks INT",
                "--periods-radius INT", "--periods-min-period INT", "--periods-min-count INT", "--periods-scope", "--periods-only"):
        assert opt in text, opt
    # the abbreviations of the options that begin with --p keep their meaning: --pair-s is --pair-stats and refuses an existing file as such
    old = tmp_path / "old.tsv"
    old.write_text("keep me\n")
    r = run_cli(["--pair-s", old, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"Pair statistics file already exists" in r.stderr
