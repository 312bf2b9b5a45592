"""Times --monomers-pileup's device path, cl_monomer_pileup_compute, beside the decomposition it follows: 1 x 1 Mbp and 10 x 1 Mbp
higher-order-repeat arrays (synth.c3_workload, the BASELINE configs[2] input) against the 12 templates they were built from (synth.hor_monomers),
one strand and both, at the default chunking.  Best of --reps after a warm-up, with the spread: align_ms and count_ms by events, the whole call by
wall clock (with the copies of the text and of the block list), and the dp_ms of the decomposition of the same input.  The cost model:
a used block of n bases against a template of L is n * L cells.  --cells N forces the cells a lane holds (CL_MONOMER_PILEUP_CELLS), --bits
lds|global where the direction bits go (CL_MONOMER_PILEUP_BITS).  --cpu runs cl_monomer_pileup_host on one core of the same host on the first
--cpu-blocks blocks and scales it by cells.  One JSON line per measurement.

    python scripts/monomer_pileup_bench.py [--cases 1x1,10x1] [--strands 1,2] [--reps 5] [--cpu] [--cells N] [--bits lds|global]
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


def used_cells(dec, lengths):
    """the cells of the blocks that take part at least_share 0: whole, no longer than two templates, score >= 0"""
    b = dec["blocks"]
    M = len(lengths)
    L = lengths[b["monomer"] % M]
    n = b["end"].astype("int64") - b["start"]
    take = (b["flags"] == 0) & (n <= 2 * L) & (b["score"] >= 0)
    return int((n[take] * L[take]).sum()), int(take.sum())


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x1,10x1")
    ap.add_argument("--strands", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=0)
    ap.add_argument("--bits", default="")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cpu-blocks", type=int, default=500)
    a = ap.parse_args()
    if a.cells:
        os.environ["CL_MONOMER_PILEUP_CELLS"] = str(a.cells)
    if a.bits:
        os.environ["CL_MONOMER_PILEUP_BITS"] = a.bits
    templates = synth.hor_monomers(SEED)
    lengths = np.array([len(t) for t in templates], dtype="int64")
    ctx = capi.Context(0)
    for case in [c for c in a.cases.split(",") if c]:
        seqs = workload(case)
        for strands in (int(x) for x in a.strands.split(",")):
            capi.monomer_decompose(ctx, seqs, templates, strands=strands)   # warm-up (code objects, pool)
            decs = [capi.monomer_decompose(ctx, seqs, templates, strands=strands) for _ in range(a.reps)]
            dec = decs[-1]
            capi.monomer_pileup(ctx, seqs, templates, dec, strands=strands)
            runs = []
            for _ in range(a.reps):
                t = time.perf_counter()
                pile = capi.monomer_pileup(ctx, seqs, templates, dec, strands=strands)
                runs.append((time.perf_counter() - t, pile["align_ms"], pile["count_ms"]))
            cells, used = used_cells(dec, lengths)
            assert used == int(pile["used"].sum())
            best = min(r[1] + r[2] for r in runs)
            dp = min(d["dp_ms"] for d in decs)
            row = {"case": case, "strands": strands, "cells_forced": a.cells, "bits": a.bits or "auto", "blocks": dec["n_blocks"], "used": used, "cells": cells,
                   "align_ms": round(min(r[1] for r in runs), 3), "count_ms": round(min(r[2] for r in runs), 3), "device_ms": round(best, 3),
                   "device_ms_spread": round(max(r[1] + r[2] for r in runs) - best, 3), "all_align_ms": [round(r[1], 3) for r in runs],
                   "call_ms": round(min(r[0] for r in runs) * 1e3, 2), "all_call_ms": [round(r[0] * 1e3, 2) for r in runs], "decompose_dp_ms": round(dp, 3),
                   "decompose_dp_ms_spread": round(max(d["dp_ms"] for d in decs) - dp, 3), "device_over_dp": round(best / dp, 4),
                   "gcells_per_s": round(cells / min(r[1] for r in runs) / 1e6, 2)}
            if a.cpu:
                part = dict(dec, blocks=dec["blocks"][:a.cpu_blocks], n_blocks=min(a.cpu_blocks, dec["n_blocks"]))
                part["seq_off"] = np.searchsorted(part["blocks"]["sequence"], np.arange(dec["n_seq"] + 1)).astype("uint64")
                t = time.perf_counter()
                capi.monomer_pileup_host(seqs, templates, part, strands=strands)
                row["cpu_s_slice"] = round(time.perf_counter() - t, 4)
                t = time.perf_counter()
                capi.monomer_pileup_host(seqs, templates, dict(part, blocks=part["blocks"][:0], n_blocks=0), strands=strands)   # the checks and the copies alone
                row["cpu_s_no_block"] = round(time.perf_counter() - t, 4)
                part_cells = used_cells(part, lengths)[0]
                row["cpu_s_scaled"] = round((row["cpu_s_slice"] - row["cpu_s_no_block"]) * cells / max(part_cells, 1), 3)
                row["cpu_over_device"] = round(row["cpu_s_scaled"] * 1e3 / best, 1)
            print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
