"""CPU suite: strand profiles, the inverted intervals read from them and the input with them turned back (cl_strands_api.cpp), and the command line
of centrolign-orient up to the point where it needs a device.  cl_strand_profile_host is held against a restatement of the definition in a dozen
lines of Python (a Counter of k-mers), cl_strand_intervals against a restatement of its rule; tests/test_gpu_strands.py holds the device path
against cl_strand_profile_host."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from centrolign_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign-orient")
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
NO_KMER, FORWARD, REVERSE, NEUTRAL = 0, 1, 2, 3
ARRAYS = ("win_off", "base_off", "kmers", "forward", "reverse")


def revcomp(s):
    s = s.encode() if isinstance(s, str) else bytes(s)
    return s.translate(COMPLEMENT)[::-1]


# ---------------------------------------------------------------- the definition, restated ------------------------------------------------------
def restated(seqs, k, W, want_votes=1):
    """the strand profile by the definition: count(x) over all sequences, the vote of every occurrence, the sums per window"""
    seqs = [s.upper() if isinstance(s, str) else bytes(s).decode().upper() for s in seqs]
    kmer_at = [{p: s[p:p + k] for p in range(len(s) - k + 1) if set(s[p:p + k]) <= set("ACGT")} for s in seqs]
    count = Counter(x for at in kmer_at for x in at.values())
    win_off = np.cumsum([0] + [(len(s) + W - 1) // W for s in seqs]).astype(np.uint64)
    base_off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    res = {name: np.zeros(int(win_off[-1]), np.uint32) for name in ("kmers", "forward", "reverse")}
    votes = np.zeros(int(base_off[-1]), np.uint8)
    for s, at in enumerate(kmer_at):
        for p, x in at.items():
            a, b = count[x], count[revcomp(x).decode()]
            vote = NEUTRAL if a + b < 2 or a == b else FORWARD if a > b else REVERSE
            votes[int(base_off[s]) + p] = vote
            g = int(win_off[s]) + p // W
            res["kmers"][g] += 1
            res["forward"][g] += vote == FORWARD
            res["reverse"][g] += vote == REVERSE
    res.update(n_seq=len(seqs), n_windows=int(win_off[-1]), n_bases=int(base_off[-1]), k=k, window=W, win_off=win_off, base_off=base_off,
               votes=votes if want_votes else None, distinct=len({min(x, revcomp(x).decode()) for x in count}))
    return res


def same_profile(got, want):
    for name in ("n_seq", "n_windows", "n_bases", "k", "window", "distinct"):
        assert got[name] == want[name], (name, got[name], want[name])
    for name in ARRAYS:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), name
    assert (got["votes"] is None) == (want["votes"] is None)
    if want["votes"] is not None:
        assert got["votes"].dtype == np.uint8 and np.array_equal(got["votes"], want["votes"])


def window_calls(profile, s):
    """True = reverse, per window of sequence s, after the inheritance rule"""
    g0, g1 = int(profile["win_off"][s]), int(profile["win_off"][s + 1])
    f, r = profile["forward"][g0:g1].astype(int), profile["reverse"][g0:g1].astype(int)
    decided = [w for w in range(g1 - g0) if f[w] != r[w]]
    calls = []
    for w in range(g1 - g0):
        left = [d for d in decided if d <= w]
        right = [d for d in decided if d > w]
        d = left[-1] if left else right[0] if right else None
        calls.append(d is not None and r[d] > f[d])
    return calls


def restated_intervals(profile, min_run=1):
    """the rule of cl_strand_intervals: rows of (sequence, start, end, windows, forward, reverse, flags)"""
    W, rows = profile["window"], []
    for s in range(profile["n_seq"]):
        b0, b1 = int(profile["base_off"][s]), int(profile["base_off"][s + 1])
        g0, length = int(profile["win_off"][s]), b1 - b0
        calls = window_calls(profile, s)
        nw = len(calls)
        v = None
        if profile["votes"] is not None:
            codes = profile["votes"][b0:b1]
            v = (codes == FORWARD).astype(int) - (codes == REVERSE).astype(int)
        prev, wa = 0, 0
        while wa < nw:
            if not calls[wa]:
                wa += 1
                continue
            wb = wa
            while wb < nw and calls[wb]:
                wb += 1
            if wb - wa >= min_run:
                start, end, flags = wa * W, min(length, wb * W), 0
                if v is not None:
                    if wa > 0:
                        lo, hi = max(prev, (wa - 1) * W), min(length, (wa + 1) * W)
                        score = [v[lo:c].sum() - v[c:hi].sum() for c in range(lo, hi + 1)]
                        start = max(c for c in range(lo, hi + 1) if score[c - lo] == max(score))
                    if wb < nw:
                        lo, hi = max(start, (wb - 1) * W), min(length, (wb + 1) * W)
                        score = [-v[lo:c].sum() + v[c:hi].sum() for c in range(lo, hi + 1)]
                        end = max(c for c in range(lo, hi + 1) if score[c - lo] == max(score))
                    flags |= 2 if wa > 0 or wb < nw else 0
                    fwd, rev = int((v[start:end] == 1).sum()), int((v[start:end] == -1).sum())
                else:
                    fwd, rev = int(profile["forward"][g0 + wa:g0 + wb].sum()), int(profile["reverse"][g0 + wa:g0 + wb].sum())
                flags |= 1 if start == 0 and end == length else 0
                rows.append((s, start, end, wb - wa, fwd, rev, flags))
                prev = end
            wa = wb
    return rows


def rows_of(intervals):
    assert intervals.dtype == capi.STRAND_INTERVAL and not intervals["reserved"].any()
    return [tuple(int(iv[name]) for name in ("sequence", "start", "end", "windows", "forward", "reverse", "flags")) for iv in intervals]


def profile_rows(profile, names):
    """cl_strand_profile_tsv, restated"""
    text = "sample\tstart\tend\tkmers\tforward\treverse\tneutral\tcall\n"
    for s, name in enumerate(names):
        g0, length = int(profile["win_off"][s]), int(profile["base_off"][s + 1] - profile["base_off"][s])
        for w, call in enumerate(window_calls(profile, s)):
            km, f, r = (int(profile[x][g0 + w]) for x in ("kmers", "forward", "reverse"))
            text += "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%s\n" % (name, w * profile["window"], min((w + 1) * profile["window"], length), km, f, r, km - f - r, "-" if call else "+")
    return text.encode()


def interval_rows(rows, names):
    """cl_strand_intervals_tsv, restated"""
    text = "sample\tstart\tend\tlength\twindows\tforward\treverse\twhole\n"
    for s, start, end, windows, f, r, flags in rows:
        text += "%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (names[s], start, end, end - start, windows, f, r, flags & 1)
    return text.encode()


def check_host(seqs, k, W):
    want = restated(seqs, k, W)
    got = capi.strand_profile_host(seqs, k=k, window=W)
    same_profile(got, want)
    assert got["sort_ms"] == 0 and got["vote_ms"] == 0
    lean = capi.strand_profile_host(seqs, k=k, window=W, want_votes=0)
    same_profile(lean, dict(want, votes=None))
    for profile in (got, lean):
        for min_run in (1, 2):
            assert rows_of(capi.strand_intervals(profile, min_run)) == restated_intervals(profile, min_run)
    return got


# ---------------------------------------------------------------- cl_strand_profile_host -------------------------------------------------------
def test_hand_cases():
    p = check_host(["AAAA", "AAAA", "TTTT"], 2, 4)
    assert p["kmers"].tolist() == [3, 3, 3] and p["forward"].tolist() == [3, 3, 0] and p["reverse"].tolist() == [0, 0, 3] and p["distinct"] == 1
    assert p["votes"].tolist() == [1, 1, 1, 0] * 2 + [2, 2, 2, 0]
    iv = capi.strand_intervals(p)
    assert rows_of(iv) == [(2, 0, 4, 1, 0, 3, capi.STRAND_WHOLE)]
    assert capi.strand_apply(["AAAA", "AAAA", "TTTT"], iv) == [b"AAAA"] * 3
    q = check_host(["AAAAC", "GTTTT"], 2, 5)   # AA / TT 3 against 3, AC / GT 1 against 1
    assert q["kmers"].tolist() == [4, 4] and not q["forward"].any() and not q["reverse"].any() and q["distinct"] == 2
    assert q["votes"].tolist() == [3, 3, 3, 3, 0] * 2 and len(capi.strand_intervals(q)) == 0


def test_palindromes_and_singletons_are_neutral():
    p = check_host(["ACGTACGTACGT"], 4, 5)   # ACGT, CGTA / TACG, GTAC: ACGT and GTAC are their own reverse complements
    assert p["votes"].tolist() == [3] * 9 + [0] * 3 and p["distinct"] == 3
    p = check_host(["ACGTACGTACGT", "ACGT"], 4, 5)   # a palindrome stays neutral however often it occurs
    assert set(p["votes"][[0, 4, 8, 12]].tolist()) == {3}
    one = check_host(["AACCA"], 3, 2)   # AAC, ACC, CCA: each once, no reverse complement anywhere
    assert one["votes"].tolist() == [3, 3, 3, 0, 0] and one["kmers"].tolist() == [2, 1, 0]
    two = check_host(["AACAAC"], 3, 6)   # AAC twice: forward; ACA, CAA once: neutral
    assert two["votes"].tolist() == [1, 3, 3, 1, 0, 0]


def messy_sequences(seed):
    """random texts over ACGTNacgtn: mostly bases, some of them copies of others or of their reverse complements, an empty one, short ones"""
    rng = np.random.default_rng(seed)
    def text(n):
        return "".join("ACGTacgtNn"[x] for x in rng.choice(10, n, p=[0.2] * 4 + [0.04] * 4 + [0.02, 0.02]))
    seqs = [text(int(n)) for n in (230, 0, 97, 3, 150)]
    seqs.append(revcomp(seqs[0][40:200]).decode())   # against two forward copies: reverse votes
    seqs.append(seqs[0][30:220])
    seqs.append(seqs[2][10:90] + revcomp(seqs[4][20:100]).decode() + seqs[2][:30])
    seqs.append("acgtn" * 9)
    return seqs


@pytest.mark.parametrize("k", [1, 2, 4, 15, 16, 17, 21, 31])
def test_random_texts(k):
    for seed, W in enumerate((1, 7, 64, 100, 2 ** 20)):
        seqs = messy_sequences(seed)
        p = check_host(seqs, k, W)
        assert p["kmers"].sum() > 0
        if k <= 17:   # (N breaks the longer k-mers of the one stretch that occurs on both strands)
            assert p["forward"].sum() > 0 and p["reverse"].sum() > 0
        if k >= 4:   # palindromes at 4 and 16, above that the k-mers of the stretches that occur once
            assert (p["votes"] == NEUTRAL).any()


def test_no_sequence_no_base_no_kmer():
    empty = check_host([], 5, 10)
    assert empty["n_seq"] == 0 and empty["n_windows"] == 0 and empty["win_off"].tolist() == [0] and len(capi.strand_intervals(empty)) == 0
    assert capi.strand_profile_tsv(empty, []) == profile_rows(empty, []) and capi.strand_apply([], capi.strand_intervals(empty)) == []
    for seqs in (["", ""], ["NNNN", "", "AC"], ["ACGT"]):
        p = check_host(seqs, 5, 3)
        assert p["kmers"].sum() == 0 and p["distinct"] == 0 and not p["votes"].any()


def test_refused_arguments():
    for kw, word in ((dict(k=0), "k"), (dict(k=32), "k"), (dict(k=-1), "k"), (dict(window=0), "window"), (dict(window=2 ** 20 + 1), "window")):
        with pytest.raises(capi.ClError) as e:
            capi.strand_profile_host(["ACGT"], **kw)
        assert e.value.code == -1 and word in str(e.value)
    capi.strand_profile_host(["ACGT"], k=31, window=2 ** 20)
    p = capi.strand_profile_host(["ACGT"], k=2, window=2)
    with pytest.raises(capi.ClError) as e:
        capi.strand_intervals(p, 0)
    assert e.value.code == -1 and "min_run" in str(e.value)
    # the lengths are added up before a base is read: the pointers below are never followed
    lib = capi.load_library()
    lib.cl_strand_profile_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(capi.StrandsParams), C.POINTER(capi.StrandProfileC)]
    lens = np.array([2 ** 29, 2 ** 29], np.uint64)
    seqs = (C.c_void_p * 2)(8, 8)
    out = capi.StrandProfileC()
    assert lib.cl_strand_profile_host(seqs, lens.ctypes.data, 2, C.byref(capi.StrandsParams(21, 1000, 1)), C.byref(out)) == -1
    assert b"lengths" in lib.cl_last_error(None) and not out.kmers


# ---------------------------------------------------------------- cl_strand_intervals -----------------------------------------------------------
def made_profile(lengths, W, forward, reverse, votes=None):
    """a profile by hand: the window counters of all sequences in one list each"""
    win_off = np.cumsum([0] + [(n + W - 1) // W for n in lengths]).astype(np.uint64)
    base_off = np.cumsum([0] + list(lengths)).astype(np.uint64)
    f, r = np.array(forward, np.uint32), np.array(reverse, np.uint32)
    assert len(f) == len(r) == win_off[-1]
    return dict(n_seq=len(lengths), n_windows=int(win_off[-1]), n_bases=int(base_off[-1]), k=3, window=W, win_off=win_off, base_off=base_off, kmers=f + r, forward=f,
                reverse=r, votes=None if votes is None else np.array(votes, np.uint8), distinct=0)


def test_undecided_windows_inherit_left_then_right():
    # sequence 0: ? ? - ? + ? -> - - - - + +; sequence 1: no decided window -> forward; sequence 2: ? + -> + +
    p = made_profile([58, 20, 20], 10, [0, 2, 1, 3, 5, 0] + [1, 0] + [0, 4], [0, 2, 4, 3, 1, 0] + [1, 0] + [0, 0])
    assert window_calls(p, 0) == [True] * 4 + [False] * 2 and window_calls(p, 1) == [False] * 2 and window_calls(p, 2) == [False] * 2
    assert rows_of(capi.strand_intervals(p)) == restated_intervals(p) == [(0, 0, 40, 4, 6, 9, 0)]
    assert capi.strand_profile_tsv(p, ["a", "b", "c"]) == profile_rows(p, ["a", "b", "c"])
    assert capi.strand_profile_tsv(p, ["a", "b", "c"]).decode().splitlines()[6] == "a\t50\t58\t0\t0\t0\t0\t+"
    # the last window is short and has no k-mer: it follows its neighbour, and the interval ends at the sequence's end
    q = made_profile([25], 10, [0, 0, 0], [3, 3, 0])
    assert rows_of(capi.strand_intervals(q)) == [(0, 0, 25, 3, 0, 6, capi.STRAND_WHOLE)]


def test_min_run_and_profiles_without_votes():
    p = made_profile([95], 10, [5, 0, 5, 0, 0, 5, 0, 0, 0, 5], [0, 5, 0, 5, 5, 0, 5, 5, 5, 0])
    for min_run, want in ((1, [(0, 10, 20, 1, 0, 5, 0), (0, 30, 50, 2, 0, 10, 0), (0, 60, 90, 3, 0, 15, 0)]), (2, [(0, 30, 50, 2, 0, 10, 0), (0, 60, 90, 3, 0, 15, 0)]),
                          (3, [(0, 60, 90, 3, 0, 15, 0)]), (4, [])):
        assert rows_of(capi.strand_intervals(p, min_run)) == restated_intervals(p, min_run) == want
    rows = restated_intervals(p)
    assert capi.strand_intervals_tsv(capi.strand_intervals(p), ["x"]) == interval_rows(rows, ["x"])
    assert capi.strand_intervals_tsv(capi.strand_intervals(p), ["x"]).decode().splitlines()[1] == "x\t10\t20\t10\t1\t0\t5\t0"
    with pytest.raises(capi.ClError) as e:
        capi.strand_intervals_tsv(capi.strand_intervals(p), [])
    assert e.value.code == -1 and "names" in str(e.value)


def votes_of(pattern):
    return [{"+": FORWARD, "-": REVERSE, ".": NEUTRAL, "0": NO_KMER}[c] for c in pattern]


def with_votes(lengths, W, pattern):
    votes = np.array(votes_of(pattern), np.uint8)
    f, r, at = [], [], 0
    for n in lengths:
        for w in range(0, n, W):
            f.append(int((votes[at + w:at + min(w + W, n)] == FORWARD).sum()))
            r.append(int((votes[at + w:at + min(w + W, n)] == REVERSE).sum()))
        at += n
    return made_profile(lengths, W, f, r, votes)


def placed(pattern, lengths=(50,)):
    """the intervals of a hand-made vote pattern at W = 10, equal to the restated rule's: (start, end, windows) of each"""
    p = with_votes(list(lengths), 10, pattern)
    rows = rows_of(capi.strand_intervals(p))
    assert rows == restated_intervals(p)
    return p, rows


def test_boundaries_from_the_votes():
    # one run inside: the neutral k-mers across each breakpoint go to the side that makes c largest
    p, rows = placed("+" * 13 + ".." + "-" * 14 + ".." + "+" * 7 + "00", [40])
    assert rows == [(0, 15, 31, 2, 0, 14, capi.STRAND_REFINED)]
    # two runs, each of one window, with a whole window between them
    p, rows = placed("+" * 10 + "-" * 10 + "+" * 10 + "-" * 10 + "+" * 10)
    assert rows == [(0, 10, 20, 1, 0, 10, 2), (0, 30, 40, 1, 0, 10, 2)]
    # the first end runs into the window between the runs
    p, rows = placed("+" * 10 + "-" * 10 + "----++++++" + "-" * 10 + "+" * 10)
    assert window_calls(p, 0) == [False, True, False, True, False] and [row[1:4] for row in rows] == [(10, 24, 1), (30, 40, 1)]
    # the second start runs into it
    p, rows = placed("+" * 10 + "-" * 8 + "++" + "+" * 6 + "----" + "-" * 10 + "+" * 10)
    assert [row[1:4] for row in rows] == [(10, 18, 1), (26, 40, 1)]
    # the window between them is reverse as well: one run
    p, rows = placed("+" * 10 + "-" * 10 + "------++++" + "-" * 10 + "+" * 10)
    assert rows == [(0, 10, 40, 3, 4, 26, 2)]
    # the whole sequence, from the votes: nothing was placed
    p, rows = placed("-" * 23 + "00" + "+" * 10 + "00", [25, 12])
    assert rows == [(0, 0, 25, 3, 0, 23, capi.STRAND_WHOLE)]
    # a run at the start, a run at the end
    p, rows = placed("-" * 12 + "+" * 16 + "-" * 10 + "00", [40])
    assert rows == [(0, 0, 12, 1, 0, 12, 2), (0, 28, 40, 1, 0, 10, 2)]
    assert capi.strand_intervals_tsv(capi.strand_intervals(p), ["s"]) == interval_rows(rows, ["s"]) == \
        b"sample\tstart\tend\tlength\twindows\tforward\treverse\twhole\ns\t0\t12\t12\t1\t0\t12\t0\ns\t28\t40\t12\t1\t0\t10\t0\n"


def test_clamp_at_the_previous_interval():
    """Runs in windows 1 and 3 of five, W = 10.  The first end, searched in [10, 30], lands at 27.  The second start is searched in [max(27, 20), 40]:
    from 20 the best c would be 23 (three forward votes in front of it), inside the first interval; from 27 it is 30"""
    p, rows = placed("+" * 10 + "-" * 10 + "+++" + "----" + "+++" + "-" * 10 + "+" * 10)
    assert window_calls(p, 0) == [False, True, False, True, False]
    assert [row[1:4] for row in rows] == [(10, 27, 1), (30, 40, 1)]
    v = (p["votes"] == FORWARD).astype(int) - (p["votes"] == REVERSE).astype(int)
    unclamped = max(range(20, 41), key=lambda c: (v[20:c].sum() - v[c:40].sum(), c))
    assert unclamped == 23
    assert capi.strand_apply(capi.strand_apply(["ACGTN" * 10], capi.strand_intervals(p)), capi.strand_intervals(p)) == [b"ACGTN" * 10]


# ---------------------------------------------------------------- cl_strand_apply ---------------------------------------------------------------
def intervals_of(rows):
    iv = np.zeros(len(rows), capi.STRAND_INTERVAL)
    for i, (s, start, end) in enumerate(rows):
        iv[i]["sequence"], iv[i]["start"], iv[i]["end"] = s, start, end
    return iv


def test_apply():
    seqs = ["AACCGGTTNNacgtRY", "", "ACGTTGCAx", "GATTACA"]
    iv = intervals_of([(0, 0, 3), (0, 3, 3), (0, 6, 16), (2, 0, 9), (3, 2, 5)])
    want = [revcomp(seqs[0][0:3]) + seqs[0][3:6].encode() + revcomp(seqs[0][6:16]), b"", revcomp(seqs[2]), b"GA" + revcomp("TTA") + b"CA"]
    assert want[0] == b"GTTCGGYRacgtNNAA" and want[2] == b"xTGCAACGT" and want[3] == b"GATAACA"   # case kept, N and other letters their own complement
    got = capi.strand_apply(seqs, iv)
    assert got == want
    assert capi.strand_apply(got, iv) == [s.encode() for s in seqs]   # an involution
    assert capi.strand_apply(seqs, intervals_of([])) == [s.encode() for s in seqs]
    # in place
    lib = capi.load_library()
    lib.cl_strand_apply.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    buf = C.create_string_buffer(seqs[0].encode(), len(seqs[0]))
    assert lib.cl_strand_apply(buf, len(seqs[0]), 0, iv.ctypes.data, len(iv), buf) == 0 and buf.raw == want[0]


@pytest.mark.parametrize("rows, word", [([(0, 5, 4)], "fit"), ([(0, 0, 9)], "fit"), ([(0, 9, 9)], "fit"), ([(0, 0, 5), (0, 4, 8)], "overlaps"),
                                        ([(0, 4, 8), (0, 0, 3)], "order"), ([(1, 0, 1), (0, 2 ** 32 - 1, 2 ** 32 - 1)], "fit")])
def test_apply_refuses(rows, word):
    with pytest.raises(capi.ClError) as e:
        capi.strand_apply(["ACGTACGT", "A"], intervals_of(rows))
    assert e.value.code == -1 and "intervals" in str(e.value) and word in str(e.value)


# ---------------------------------------------------------------- inversions and flips in HOR arrays --------------------------------------------
def recipe(seed):
    """hor_sequences(seed, 20000, 4) with an inner inversion in one sequence and another one flipped whole: (original, modified, i, (B, E), j)"""
    rng = np.random.default_rng(seed)
    orig = [s.encode() for s in synth.hor_sequences(seed, 20000, 4)]
    i = int(rng.integers(0, 4))
    B = int(rng.integers(1000, len(orig[i]) - 9000))
    E = B + int(rng.integers(1500, 8000))
    j = (i + 1 + int(rng.integers(0, 3))) % 4
    mod = list(orig)
    mod[i] = orig[i][:B] + revcomp(orig[i][B:E]) + orig[i][E:]
    mod[j] = revcomp(orig[j])
    return orig, mod, i, (B, E), j


# seed: the inner inversion as made, as cl_strand_profile_host + cl_strand_intervals find it at k = 21, W = 1000
RECIPE = {0: ((4737, 9559), (4737, 9559)), 1: ((6115, 12523), (6114, 12523)), 2: ((4685, 6895), (4685, 6895)), 3: ((1855, 4521), (1855, 4521)),
          4: ((6583, 13812), (6615, 13812)), 5: ((9050, 10697), (9050, 10697)), 6: ((6380, 11245), (6380, 11244)), 7: ((4675, 10622), (4691, 10621)),
          8: ((5617, 8641), (5615, 8641)), 9: ((9705, 17451), (9711, 17460))}
RESTORED = (0, 2, 3, 5)   # the seeds whose inner inversion comes back to the base


def check_recipe(seed, profile_of):
    """the conditions on the recipe's result, for the host and the device profile alike"""
    orig, mod, i, truth, j = recipe(seed)
    assert truth == RECIPE[seed][0]
    profile = profile_of(mod)
    iv = capi.strand_intervals(profile)
    rows = rows_of(iv)
    assert [row[0] for row in rows] == sorted([i, j]), rows
    whole, inner = (rows[0], rows[1]) if j < i else (rows[1], rows[0])
    assert whole[:3] == (j, 0, len(orig[j])) and whole[6] == capi.STRAND_WHOLE          # every whole flip exactly
    assert abs(inner[1] - truth[0]) <= 64 and abs(inner[2] - truth[1]) <= 64, (inner, truth)   # every boundary within 64 bases
    assert inner[1:3] == RECIPE[seed][1] and inner[6] == capi.STRAND_REFINED
    fixed = capi.strand_apply(mod, iv)
    assert fixed[j] == orig[j]
    assert (fixed[i] == orig[i]) == (seed in RESTORED)
    assert all(fixed[s] == orig[s] for s in range(4) if s not in (i, j))
    return profile, iv


@pytest.mark.parametrize("seed", range(10))
def test_recipe(seed):
    check_recipe(seed, lambda seqs: capi.strand_profile_host(seqs, k=21, window=1000))


@pytest.mark.parametrize("seed", range(5))
def test_unmodified_arrays_have_no_interval(seed):
    p = capi.strand_profile_host(synth.hor_sequences(seed, 20000, 4), k=21, window=1000)
    assert len(capi.strand_intervals(p)) == 0 and not p["reverse"].any() and not (p["votes"] == REVERSE).any() and p["forward"].sum() > 50000


def test_one_sequence_alone():
    (seq,) = synth.hor_sequences(11, 40000, 1)
    seq = seq.encode()
    mod = seq[:12345] + revcomp(seq[12345:18000]) + seq[18000:]
    rows = rows_of(capi.strand_intervals(capi.strand_profile_host([mod], k=21, window=1000)))
    assert len(rows) == 1 and rows[0][1:3] == (12345, 18008)
    assert abs(rows[0][1] - 12345) <= 64 and abs(rows[0][2] - 18000) <= 64


# ---------------------------------------------------------------- the interface ----------------------------------------------------------------
def test_abi():
    lib = capi.load_library()
    new = ["cl_strands_params_default", "cl_strand_profile_host", "cl_strand_profile_compute", "cl_strand_profile_free", "cl_strand_intervals",
           "cl_strand_intervals_free", "cl_strand_apply", "cl_strand_profile_tsv", "cl_strand_intervals_tsv"]
    for sym in new:
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    lib.cl_abi_version.restype = C.c_int
    assert lib.cl_abi_version() == 22 and capi.ABI_VERSION == 22
    # the header's layouts by hand (LP64): {3 x 4 bytes}, {3 x u64, 2 x 4 bytes, 6 pointers, u64, 2 floats}, {8 x u32}
    sizes_by_hand = [12, 96, 32]
    assert [C.sizeof(capi.StrandsParams), C.sizeof(capi.StrandProfileC), C.sizeof(capi.StrandIntervalC)] == sizes_by_hand
    assert capi.STRAND_INTERVAL.itemsize == 32
    p = capi.StrandsParams()
    lib.cl_strands_params_default(C.byref(p))
    assert (p.k, p.window, p.want_votes) == (21, 1000, 1)
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is not None:
        src = ('#include <stdio.h>\n#include "centrolign_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(cl_strands_params), sizeof(cl_strand_profile), '
               'sizeof(cl_strand_interval)); return 0; }\n')
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "s.c"), "w") as f:
                f.write(src)
            subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "s"), os.path.join(d, "s.c")], check=True)
            sizes = [int(x) for x in subprocess.run([os.path.join(d, "s")], check=True, capture_output=True, text=True).stdout.split()]
        assert sizes == sizes_by_hand


# ---------------------------------------------------------------- the command line --------------------------------------------------------------
def run_cli(args, **kw):
    return subprocess.run([BIN] + [str(a) for a in args], capture_output=True, timeout=60, **kw)


@pytest.fixture()
def fasta(tmp_path):
    p = tmp_path / "in.fa"
    p.write_text(">a\nACGTACGTACGTACGTACGTACGTACGT\n>b\nACGTACGAACGTACGTACGTACGTACGT\n")
    return p


def test_cli_help():
    r = run_cli(["-h"])
    assert r.returncode == 0 and r.stdout == b""
    usage = r.stderr.decode()
    assert usage.startswith("Usage: centrolign-orient [options] sequences.fasta")
    for word in (" -k INT", "--window / -w INT", "--min-run INT", "--profile FILE", "--fasta-out FILE", "--devices LIST", " -v INT", " -h ", "[21]", "[1000]"):
        assert word in usage, word


def test_cli_refusals(tmp_path, fasta):
    """each is one "error:" line and status 1 with nothing on standard output, before the FASTA is read or a device opened"""
    old = tmp_path / "old.tsv"
    old.write_text("keep me\n")
    out = tmp_path / "out.tsv"
    cases = {
        "an existing profile": (["--profile", old, fasta], "--profile file already exists: %s" % old),
        "an existing FASTA": (["--fasta-out", old, fasta], "--fasta-out file already exists: %s" % old),
        "one file for both": (["--profile", out, "--fasta-out", out, fasta], "--profile and --fasta-out name the same file"),
        "no FASTA": (["-k", 5], "no FASTA file was given (-h shows the options)"),
        "two FASTAs": ([fasta, fasta], "more than one FASTA file was given"),
        "an unknown option": (["--periods", out, fasta], "unknown option --periods"),
        "an option without its value": ([fasta, "--profile"], "option --profile needs a value"),
        "--devices": (["--devices", "0,x", fasta], "--devices expects comma-separated device ordinals, got '0,x'"),
        "-v": (["-v", "loud", fasta], "-v expects a whole number, got 'loud'"),
    }
    for opt, what, bad in (("-k", "a whole number from 1 to 31", (0, 32, "x", "-3", "2.5", "")), ("-w", "a whole number from 1 to 1048576", (0, 2 ** 20 + 1, "x", "-3", "1e3")),
                           ("--window", "a whole number from 1 to 1048576", (0,)), ("--min-run", "a whole number from 1 to 4294967295", (0, 2 ** 32, "x", "-1", "1.5"))):
        for value in bad:
            cases["%s %s" % (opt, value)] = ([opt, value, "--profile", out, fasta], "%s expects %s, got '%s'" % ("--window" if opt == "-w" else opt, what, value))
    assert len(cases) >= 25
    for name, (args, message) in cases.items():
        r = run_cli(args)
        assert r.returncode == 1 and r.stdout == b"", (name, r.returncode, r.stderr)
        assert r.stderr.decode() == "error: %s\n" % message, (name, r.stderr)
        assert not out.exists() and old.read_text() == "keep me\n", name
    # the same refusals without a FASTA that could be read: they come first
    r = run_cli(["-k", 40, tmp_path / "missing.fa"])
    assert r.returncode == 1 and b"-k expects" in r.stderr and b"missing.fa" not in r.stderr
    # the largest values pass the option checks: the run then ends at the FASTA that is not there, or at one that is none, without a device
    args = ["-k", 31, "-w", 2 ** 20, "--min-run", 2 ** 32 - 1, "--profile", out, "--fasta-out", tmp_path / "fixed.fa", "--devices", "0,1", "-v", 3]
    r = run_cli(args + [tmp_path / "missing.fa"])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.decode() == "error: Could not open file %s\n" % (tmp_path / "missing.fa")
    r = run_cli(args + [old])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"error: ") and b"GPU" not in r.stderr and not out.exists()
    r = run_cli(args + ["-"], input=b"no fasta\n")
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"error: ") and b"GPU" not in r.stderr
