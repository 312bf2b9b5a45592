"""Times --dotplot's device path, cl_kmer_dotplot_compute, at the defaults (k 21, windows of 2 000 bases, 86 %): 1 x 1 Mbp with pairs of one
sequence ("self") and 10 x 1 Mbp with all pairs (synth.c3_workload, the BASELINE configs[2] input).  Best of --reps after a warm-up: the two
device phases by events, the whole call by wall clock.  Two comparisons:
  * the numpy restatement of tests/test_dotplot.py on one core of the same host: np.unique per window for all windows, np.intersect1d for a
    sample of --cpu-pairs window pairs, scaled to all of them;
  * the only route to such numbers on a device before this kernel: cl_kmer_distances_compute with the 500 windows of the 1 x 1 Mbp input
    passed as 500 sequences (each window with the k - 1 bases its last k-mers reach into), its pairs_ms — multiset sums rather than set
    sizes, the same shape of work.
One JSON line per input and one for the route through cl_kmer_distances_compute.

    python scripts/dotplot_bench.py [--cases 1x1,10x1] [--reps 3] [--cpu] [--cpu-pairs 2000] [--no-distances]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from centrolign_amd import capi, synth  # noqa: E402

K, W, MIN_IDENTITY = 21, 2000, 86.0


def workload(case):
    n, mbp = (int(x) for x in case.split("x"))
    names, seqs, _ = synth.c3_workload(length=mbp * 1000000, n_seq=n)
    return [seqs[nm] for nm in names]


def spread(values):
    return round(max(values) - min(values), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x1,10x1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-pairs", type=int, default=2000)
    ap.add_argument("--no-distances", action="store_true")
    a = ap.parse_args()
    ctx = capi.Context(0)
    for case in a.cases.split(","):
        seqs = workload(case)
        pairs = "self" if len(seqs) == 1 else "all"
        capi.kmer_dotplot(ctx, seqs, pairs=pairs)   # warm-up (code objects, pool)
        runs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            plot = capi.kmer_dotplot(ctx, seqs, pairs=pairs)
            runs.append((time.perf_counter() - t, plot["spectra_ms"], plot["pairs_ms"]))
        best = tuple(min(r[i] for r in runs) for i in range(3))
        G = plot["n_windows"]
        d = plot["distinct"].astype(np.float64)
        n_pairs = G * (G + 1) // 2
        # the cost model of the pair phase: every element of a row list is looked up in every column list, ceil(log2(|B| + 1)) LDS reads each
        steps = np.ceil(np.log2(np.maximum(d, 1) + 1))
        lds_reads = float(d @ np.cumsum(steps[::-1])[::-1])   # pairs a <= b (with pairs of one sequence and one sequence: the same pairs)
        row = {"case": case, "pairs": pairs, "k": K, "window": W, "min_identity": MIN_IDENTITY, "windows": G, "window_pairs": n_pairs, "entries": len(plot["entries"]),
               "call_ms": round(best[0] * 1e3, 2), "spectra_ms": round(best[1], 3), "pairs_ms": round(best[2], 3),
               "all_call_ms": [round(r[0] * 1e3, 2) for r in runs], "all_pairs_ms": [round(r[2], 3) for r in runs], "pairs_ms_spread": spread([r[2] for r in runs]),
               "ns_per_window_pair": round(best[2] * 1e6 / n_pairs, 2), "lds_reads_model": lds_reads,
               "lds_reads_per_window_pair": round(lds_reads / n_pairs, 1), "lds_TB_per_s": round(lds_reads * 4 / (best[2] * 1e-3) / 1e12, 2)}
        if a.cpu:
            from tests.test_dotplot import window_sets
            t = time.perf_counter()
            _, sets = window_sets(seqs, K, W)
            row["cpu_windows_s"] = round(time.perf_counter() - t, 2)
            rng = np.random.default_rng(1)
            sample = [(int(x), int(y)) for x, y in zip(rng.integers(0, G, a.cpu_pairs), rng.integers(0, G, a.cpu_pairs))]
            t = time.perf_counter()
            for x, y in sample:
                len(np.intersect1d(sets[x], sets[y], assume_unique=True))
            row["cpu_pairs_s_scaled"] = round((time.perf_counter() - t) * n_pairs / len(sample), 2)
            row["cpu_pairs_sampled"] = len(sample)
            assert np.array_equal(plot["distinct"], np.array([len(x) for x in sets], np.uint32))
        print(json.dumps(row), flush=True)
        if case == "1x1" and not a.no_distances:
            s = seqs[0]
            windows = [s[w * W:(w + 1) * W + K - 1] for w in range(G)]
            capi.kmer_distances(ctx, windows, k=K)
            druns = []
            for _ in range(a.reps):
                t = time.perf_counter()
                total, shared, _, times = capi.kmer_distances(ctx, windows, k=K, want_times=True)
                druns.append((time.perf_counter() - t, times["spectra_ms"], times["pairs_ms"]))
            dbest = min(druns, key=lambda r: r[2])
            print(json.dumps({"case": "1x1 as %d sequences through cl_kmer_distances_compute" % G, "call_ms": round(min(r[0] for r in druns) * 1e3, 2),
                              "spectra_ms": round(dbest[1], 3), "pairs_ms": round(dbest[2], 3), "all_pairs_ms": [round(r[2], 3) for r in druns],
                              "pairs_ms_spread": spread([r[2] for r in druns]), "dotplot_pairs_ms": row["pairs_ms"],
                              "dotplot_faster_by": round(dbest[2] / best[2], 2),
                              "faster_by_more_than_both_spreads": bool(dbest[2] - best[2] > max(spread([r[2] for r in druns]), row["pairs_ms_spread"]))}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
