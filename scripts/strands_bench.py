"""Times the strand profile's device path, cl_strand_profile_compute, at the defaults (k 21, windows of 1 000 bases): 1 x 1 Mbp and 10 x 1 Mbp
(synth.c3_workload, the BASELINE configs[2] input).  Best of --reps after a warm-up, with the spread: the two device phases by events and the
whole call by wall clock, with the votes copied back (want_votes 1) and without.  The yardstick is the existing pipeline of the same shape, the link
phase of cl_period_spectrum_compute at the same k on the same input in the same process (links_ms: one 42-bit sort of every k-mer position plus
linear passes): the profile's device time is to stay within twice that.  --cpu runs cl_strand_profile_host on one core of the same host and
compares every array.  One JSON line per input.

    python scripts/strands_bench.py [--cases 1x1,10x1] [--reps 5] [--cpu]
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


def workload(case):
    """NxM: N sequences of M Mbp of synth.c3_workload"""
    n, mbp = (int(x) for x in case.split("x"))
    names, seqs, _ = synth.c3_workload(length=mbp * 1000000, n_seq=n)
    return [seqs[nm] for nm in names]


def spread(values):
    return round(max(values) - min(values), 3)


def timed(reps, call, times):
    call()   # warm-up (code objects, pool)
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        res = call()
        runs.append((time.perf_counter() - t,) + tuple(res[name] for name in times))
    return res, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x1,10x1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    ctx = capi.Context(0)
    for case in a.cases.split(","):
        seqs = workload(case)
        pr, runs = timed(a.reps, lambda: capi.strand_profile(ctx, seqs), ("sort_ms", "vote_ms"))
        _, lean = timed(a.reps, lambda: capi.strand_profile(ctx, seqs, want_votes=0), ("sort_ms", "vote_ms"))
        _, periods = timed(a.reps, lambda: capi.period_spectrum(ctx, seqs, k=pr["k"], want_hist=0), ("links_ms",))
        device = [r[1] + r[2] for r in runs]
        yardstick = min(r[1] for r in periods)
        row = {"case": case, "k": pr["k"], "window": pr["window"], "bases": pr["n_bases"], "windows": pr["n_windows"], "occurrences": int(pr["kmers"].sum()),
               "distinct": pr["distinct"], "forward": int(pr["forward"].sum()), "reverse": int(pr["reverse"].sum()), "intervals": len(capi.strand_intervals(pr)),
               "sort_ms": round(min(r[1] for r in runs), 3), "vote_ms": round(min(r[2] for r in runs), 3), "device_ms": round(min(device), 3),
               "device_ms_spread": spread(device), "all_sort_ms": [round(r[1], 3) for r in runs], "all_vote_ms": [round(r[2], 3) for r in runs],
               "call_ms": round(min(r[0] for r in runs) * 1e3, 2), "all_call_ms": [round(r[0] * 1e3, 2) for r in runs],
               "call_ms_without_votes": round(min(r[0] for r in lean) * 1e3, 2),
               "periods_links_ms": round(yardstick, 3), "all_periods_links_ms": [round(r[1], 3) for r in periods],
               "device_over_periods_links": round(min(device) / yardstick, 3), "within_twice": bool(min(device) <= 2 * yardstick)}
        if a.cpu:
            t = time.perf_counter()
            host = capi.strand_profile_host(seqs)
            row["host_s"] = round(time.perf_counter() - t, 2)
            same = all(np.array_equal(host[name], pr[name]) for name in ("win_off", "base_off", "kmers", "forward", "reverse", "votes")) and host["distinct"] == pr["distinct"]
            row["host_equal"] = bool(same)
            row["host_over_call"] = round(row["host_s"] * 1e3 / row["call_ms"], 1)
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
