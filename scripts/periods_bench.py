"""Times --periods' device path, cl_period_spectrum_compute, at the defaults (k 8, windows of 10 000 bases, periods up to 8 000, 3 peaks): 1 x 1 Mbp
and 10 x 1 Mbp (synth.c3_workload, the BASELINE configs[2] input).  Best of --reps after a warm-up: the two device phases by events, the whole
call by wall clock, each with the rows copied back (want_hist 1) and without (want_hist 0).  The cost model of the histogram phase:
every occurrence is read once (4 bytes) and is one LDS add; every row is zeroed, written and read back twice (totals, peaks), (D + 1) * 4 bytes
each time.  --cpu runs the numpy restatement of tests/test_periods.py on one core of the same host.  One JSON line per input.

    python scripts/periods_bench.py [--cases 1x1,10x1] [--reps 3] [--cpu]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from centrolign_amd import capi, synth  # noqa: E402


def workload(case):
    """NxM: N sequences of M Mbp of synth.c3_workload; horNxM: of synth.hor_sequences (12 x 171 arrays: 4 links in 10 fall on one period);
    monoNxM: one base repeated, every link in bin 1 (the most contention an input can cause)"""
    kind = case.rstrip("0123456789x")
    n, mbp = (int(x) for x in case[len(kind):].split("x"))
    if kind == "hor":
        return synth.hor_sequences(41, mbp * 1000000, n)
    if kind == "mono":
        return ["A" * (mbp * 1000000)] * n
    names, seqs, _ = synth.c3_workload(length=mbp * 1000000, n_seq=n)
    return [seqs[nm] for nm in names]


def spread(values):
    return round(max(values) - min(values), 3)


def timed(ctx, seqs, reps, **kw):
    capi.period_spectrum(ctx, seqs, **kw)   # warm-up (code objects, pool)
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        sp = capi.period_spectrum(ctx, seqs, **kw)
        runs.append((time.perf_counter() - t, sp["links_ms"], sp["hist_ms"]))
    return sp, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x1,10x1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true")
    a = ap.parse_args()
    ctx = capi.Context(0)
    for case in a.cases.split(","):
        seqs = workload(case)
        sp, runs = timed(ctx, seqs, a.reps)
        _, lean = timed(ctx, seqs, a.reps, want_hist=0)
        G, R, D = sp["n_windows"], sp["n_rows"], sp["max_period"]
        occurrences = int(sp["kmers"][G:].sum())
        links = int(sp["links"][G:].sum())
        best_hist = min(r[2] for r in runs)
        top = sp["peaks"][G:, 0]
        row = {"case": case, "k": sp["k"], "window": sp["window"], "max_period": D, "windows": G, "rows": R, "occurrences": occurrences, "links": links,
               "top_periods": [int(p["period"]) for p in top], "top_share": [round(float(p["count"]) / max(int(l), 1), 3) for p, l in zip(top, sp["links"][G:])],
               "call_ms": round(min(r[0] for r in runs) * 1e3, 2), "links_ms": round(min(r[1] for r in runs), 3), "hist_ms": round(best_hist, 3),
               "all_call_ms": [round(r[0] * 1e3, 2) for r in runs], "all_links_ms": [round(r[1], 3) for r in runs], "all_hist_ms": [round(r[2], 3) for r in runs],
               "hist_ms_spread": spread([r[2] for r in runs]),
               "call_ms_without_rows": round(min(r[0] for r in lean) * 1e3, 2), "all_call_ms_without_rows": [round(r[0] * 1e3, 2) for r in lean],
               "model_bytes_read": occurrences * 4 + 2 * R * (D + 1) * 4, "model_bytes_written": R * (D + 1) * 4, "model_lds_adds": occurrences,
               "ns_per_occurrence_hist": round(best_hist * 1e6 / max(occurrences, 1), 3)}
        if a.cpu:
            from tests.test_periods import restated, same_spectrum
            t = time.perf_counter()
            want = restated(seqs, sp["k"], sp["window"], D)
            row["cpu_s"] = round(time.perf_counter() - t, 2)
            same_spectrum(sp, want)
            row["cpu_over_call"] = round(row["cpu_s"] * 1e3 / row["call_ms"], 1)
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
