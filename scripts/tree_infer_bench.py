"""Times --infer-tree's parts: cl_kmer_distances_compute (device spectra and all-pairs sums, by events, and the whole call) and the host's
neighbor joining, at 10 x 1 Mbp (BASELINE configs[2] input), 50 x 1 Mbp and 50 x 5 Mbp, with the pair phase against its traffic model
(N - 1) * sum_i |distinct_i| * 12 B.  --cpu also times the numpy restatement of the spectra and pair sums (tests/test_gpu_tree_infer.py) on
the same input; at 50 x 5 Mbp its pair phase is timed on --cpu-pairs pairs and scaled to all of them.  One JSON line per input.

    python scripts/tree_infer_bench.py [--cases 10x1,50x1,50x5] [--k 21] [--reps 3] [--cpu] [--cpu-pairs 40]
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


def fast_hor_family(seed, length, n_seq, mono_len=171, hor_n=12, mono_div=0.25, hor_div=0.02, seq_div=0.005):
    """HOR arrays like synth.hor_sequences (substitutions and single-base indels, vectorised) for inputs too large for the per-base generator"""
    rng = np.random.default_rng(seed)

    def mutate(s, r):
        x = rng.random(len(s))
        out = s.copy()
        sub = x < r * 0.8
        out[sub] = rng.integers(0, 4, int(sub.sum()), dtype=np.uint8)
        keep = ~((x >= r * 0.8) & (x < r * 0.9))
        ins = (x >= r * 0.9) & (x < r)
        rep = np.where(ins, 2, 1)[keep]
        out = np.repeat(out[keep], rep)
        return out

    mono = rng.integers(0, 4, mono_len, dtype=np.uint8)
    hor = np.concatenate([mutate(mono, mono_div) for _ in range(hor_n)])
    anc = np.concatenate([mutate(hor, hor_div) for _ in range(length // len(hor) + 1)])[:length]
    letters = np.frombuffer(b"ACGT", np.uint8)
    return [letters[mutate(anc, seq_div)].tobytes().decode() for _ in range(n_seq)]


def workload(case):
    n, mbp = (int(x) for x in case.split("x"))
    if (n, mbp) == (10, 1):
        names, seqs, _ = synth.c3_workload()
        return [seqs[nm] for nm in names]
    return fast_hor_family(7 + n + mbp, mbp * 1000000, n)


def numpy_pairs(spec, pairs):
    t = time.perf_counter()
    for i, j in pairs:
        _, a, b = np.intersect1d(spec[i][0], spec[j][0], assume_unique=True, return_indices=True)
        int(np.minimum(spec[i][1][a], spec[j][1][b]).sum())
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="10x1,50x1,50x5")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-pairs", type=int, default=40)
    a = ap.parse_args()
    ctx = capi.Context(0)
    for case in a.cases.split(","):
        t = time.perf_counter()
        seqs = workload(case)
        gen_s = time.perf_counter() - t
        n = len(seqs)
        capi.kmer_distances(ctx, seqs, k=a.k)   # warm-up (code objects, pool)
        runs = []
        for _ in range(a.reps):
            t = time.perf_counter()
            total, shared, distance, times = capi.kmer_distances(ctx, seqs, k=a.k, want_times=True)
            runs.append((time.perf_counter() - t, times["spectra_ms"], times["pairs_ms"]))
        best = min(runs)
        names = ["s%d" % i for i in range(n)]
        t = time.perf_counter()
        capi.neighbor_joining_newick(distance, names)
        nj_ms = (time.perf_counter() - t) * 1e3
        # distinct list sizes for the traffic model: one more call on the host side of the spectra is not needed, the numpy restatement gives them
        from tests.test_gpu_tree_infer import spectrum
        t = time.perf_counter()
        spec = [spectrum(s, a.k) for s in seqs]
        cpu_spectra_s = time.perf_counter() - t
        distinct = sum(len(u) for u, _ in spec)
        traffic = (n - 1) * distinct * 12
        row = {"case": case, "k": a.k, "n": n, "bases": int(sum(len(s) for s in seqs)), "generate_s": round(gen_s, 2),
               "call_ms": round(best[0] * 1e3, 2), "spectra_ms": round(best[1], 2), "pairs_ms": round(best[2], 2), "nj_ms": round(nj_ms, 3),
               "distinct_total": distinct, "pair_traffic_GB": round(traffic / 1e9, 3), "pair_GB_per_s": round(traffic / (best[2] * 1e-3) / 1e9, 1),
               "all_call_ms": [round(r[0] * 1e3, 2) for r in runs]}
        if a.cpu:
            pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
            want_total = np.array([int(c.sum()) for _, c in spec], np.uint64)
            row["cpu_spectra_s"] = round(cpu_spectra_s, 2)
            if len(pairs) > a.cpu_pairs and case == "50x5":
                step = len(pairs) // a.cpu_pairs
                sample = pairs[::step][:a.cpu_pairs]
                row["cpu_pairs_s_scaled"] = round(numpy_pairs(spec, sample) * len(pairs) / len(sample), 1)
                row["cpu_pairs_sampled"] = len(sample)
            else:
                row["cpu_pairs_s"] = round(numpy_pairs(spec, pairs), 2)
                for i, j in pairs[:: max(1, len(pairs) // 20)]:   # spot check against the device
                    _, x, y = np.intersect1d(spec[i][0], spec[j][0], assume_unique=True, return_indices=True)
                    assert int(np.minimum(spec[i][1][x], spec[j][1][y]).sum()) == int(shared[i, j])
            assert np.array_equal(want_total, total)
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
