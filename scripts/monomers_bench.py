"""Times --monomers' device path, cl_monomer_decompose_compute: 1 x 1 Mbp and 10 x 1 Mbp higher-order-repeat arrays (synth.c3_workload, the
BASELINE configs[2] input) against the 12 templates they were built from (synth.hor_monomers), one strand and both, at every --chunkings pair.
Best of --reps after a warm-up: the two device phases by events, the whole call by wall clock, with the spread.  The cost model: every
row of every problem is one step of the kernel over all template cells, cells = rows * template bases.  --rowstep times one problem of
--rowstep-bases rows (chunk 0): device time / rows is the kernel's time per row.  --cells N forces the cells a lane holds (CL_MONOMERS_CELLS).
--cpu runs cl_monomer_decompose_host on one core of the same host on the first --cpu-bases bases of the first sequence, scales it by cells, and
checks there that the chunked blocks equal the unchunked ones.  One JSON line per measurement.

    python scripts/monomers_bench.py [--cases 1x1,10x1] [--strands 1,2] [--chunkings 2048:512,4096:512,8192:1024] [--reps 3] [--cpu] [--rowstep]
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from centrolign_amd import capi, synth  # noqa: E402

SEED = 7   # synth.c3_workload's


def workload(case):
    n, mbp = (int(x) for x in case.split("x"))
    names, seqs, _ = synth.c3_workload(length=mbp * 1000000, n_seq=n, seed=SEED)
    return [seqs[nm] for nm in names]


def rows_of(seqs, chunk, overlap):
    """the rows of all problems: what the chunks' overlaps add to the bases"""
    if chunk == 0:
        return sum(len(s) for s in seqs)
    return sum(min(len(s), (c + 1) * chunk + overlap) - max(0, c * chunk - overlap) for s in seqs for c in range((len(s) + chunk - 1) // chunk))


def timed(ctx, seqs, templates, reps, **kw):
    capi.monomer_decompose(ctx, seqs, templates, **kw)   # warm-up (code objects, pool)
    runs = []
    for _ in range(reps):
        t = time.perf_counter()
        dec = capi.monomer_decompose(ctx, seqs, templates, **kw)
        runs.append((time.perf_counter() - t, dec["dp_ms"], dec["trace_ms"]))
    return dec, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x1,10x1")
    ap.add_argument("--strands", default="1,2")
    ap.add_argument("--chunkings", default="2048:512,4096:512,8192:1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-bases", type=int, default=40000)
    ap.add_argument("--rowstep", action="store_true")
    ap.add_argument("--rowstep-bases", type=int, default=100000)
    a = ap.parse_args()
    if a.cells:
        os.environ["CL_MONOMERS_CELLS"] = str(a.cells)
    templates = synth.hor_monomers(SEED)
    bases = sum(len(t) for t in templates)
    ctx = capi.Context(0)
    chunkings = [tuple(int(x) for x in pair.split(":")) for pair in a.chunkings.split(",")]
    for case in [c for c in a.cases.split(",") if c]:
        seqs = workload(case)
        for strands in (int(x) for x in a.strands.split(",")):
            for chunk, overlap in chunkings:
                dec, runs = timed(ctx, seqs, templates, a.reps, chunk=chunk, overlap=overlap, strands=strands)
                rows = rows_of(seqs, chunk, overlap)
                cells = rows * bases * strands
                best_dp = min(r[1] for r in runs)
                row = {"case": case, "strands": strands, "chunk": chunk, "overlap": overlap, "cells_forced": a.cells, "problems": dec["n_problems"], "blocks": dec["n_blocks"],
                       "rows": rows, "cells": cells, "call_ms": round(min(r[0] for r in runs) * 1e3, 2), "dp_ms": round(best_dp, 3),
                       "trace_ms": round(min(r[2] for r in runs), 3), "all_call_ms": [round(r[0] * 1e3, 2) for r in runs], "all_dp_ms": [round(r[1], 3) for r in runs],
                       "dp_ms_spread": round(max(r[1] for r in runs) - best_dp, 3), "gcells_per_s": round(cells / best_dp / 1e6, 2)}
                if a.cpu:
                    part = [seqs[0][:a.cpu_bases]]
                    t = time.perf_counter()
                    host = capi.monomer_decompose_host(part, templates, chunk=chunk, overlap=overlap, strands=strands)
                    row["cpu_s_slice"] = round(time.perf_counter() - t, 3)
                    whole = capi.monomer_decompose_host(part, templates, chunk=0, strands=strands)
                    row["slice_equals_whole"] = bool(host["n_blocks"] == whole["n_blocks"] and (host["blocks"] == whole["blocks"]).all())
                    row["cpu_s_scaled"] = round(row["cpu_s_slice"] * rows / rows_of(part, chunk, overlap), 2)
                    row["cpu_over_call"] = round(row["cpu_s_scaled"] * 1e3 / row["call_ms"], 1)
                print(json.dumps(row), flush=True)
    if a.rowstep:
        seq = workload("1x1")[0][:a.rowstep_bases]
        for strands in (int(x) for x in a.strands.split(",")):
            dec, runs = timed(ctx, [seq], templates, a.reps, chunk=0, strands=strands)
            best = min(r[1] for r in runs)
            print(json.dumps({"case": "rowstep", "strands": strands, "cells_forced": a.cells, "rows": len(seq), "template_bases": bases * strands, "dp_ms": round(best, 3),
                              "all_dp_ms": [round(r[1], 3) for r in runs], "us_per_row": round(best * 1e3 / len(seq), 4)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
