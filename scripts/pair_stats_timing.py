"""What the pairwise statistics cost: one cl_induced_pairwise_stats call against the only way to the same numbers before it existed —
cl_induced_pairwise_cigars plus a host parse of its text — on the root graph of BASELINE configs[2] (10 x 1 Mbp, made by cl_msa in the same
run), for its 45 pairs and for the 45 repeated to 1 225, several times each in the same process, alternating.  Wall times (the calls end in a
device synchronise).  Writes one JSON record (--out FILE, default standard output).

usage:  python scripts/pair_stats_timing.py [--length 1000000] [--repeats 7] [--out FILE] [--calls-only]
        python scripts/pair_stats_timing.py --add-kernels KERNEL_TRACE.csv --out FILE
Device (kernel) time: run it once of its own with --calls-only (one call of each kind per pair count) under rocprofv3 --kernel-trace, then
--add-kernels puts the kernels' durations from that trace (dispatches told apart by kernel name and grid size = pairs x 1024) into FILE's
"kernels" entry; that step needs no device.  profiles/pair_stats_timing.json is the record of the first form with the second applied.
"""
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centrolign_amd import capi, synth  # noqa: E402

OPS = {b"="[0]: 0, b"X"[0]: 1, b"I"[0]: 2, b"D"[0]: 3}
RUN = re.compile(rb"(\d+)([=XID])")


def parse(cigar):
    """[eq, x, ins, del, eq_runs, x_runs, ins_runs, del_runs] of one CIGAR text"""
    out = [0] * 8
    for n, c in RUN.findall(cigar):
        k = OPS[c[0]]
        out[k] += int(n)
        out[4 + k] += 1
    return out


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def add_kernels(trace_csv, out_file):
    """per pair count the device time of the stats kernel and of the two passes of the CIGAR kernel, from a rocprofv3 kernel trace of --calls-only"""
    rows = list(csv.DictReader(open(trace_csv)))
    rec = json.load(open(out_file))
    kernels = {}
    for tag in ("45", "1225"):
        k = {}
        for r in rows:
            name = r["Kernel_Name"]
            grid, wg = int(r.get("Grid_Size_X") or r["Grid_Size"]), int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
            if "induced_" not in name or grid // wg != int(tag) or wg != 1024:
                continue
            key = "stats_kernel_ms" if "induced_stats_kernel" in name else "cigar_write_pass_ms" if "<true>" in name or "Lb1" in name else "cigar_count_pass_ms"
            k[key] = round(k.get(key, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6, 3)
        if "cigar_count_pass_ms" in k and "cigar_write_pass_ms" in k:
            k["cigar_kernels_ms"] = round(k["cigar_count_pass_ms"] + k["cigar_write_pass_ms"], 3)
        for side in ("stats", "cigars"):
            ms = k.get("stats_kernel_ms" if side == "stats" else "cigar_kernels_ms")
            if ms:
                k["GB_per_s_" + side] = round(rec["timing"]["pairs_" + tag]["bytes_min_" + side] / ms / 1e6, 1)
        kernels[tag] = k
    rec["kernels"] = kernels
    rec["kernels_command"] = "rocprofv3 --kernel-trace -- python scripts/pair_stats_timing.py --calls-only (a run of its own), then --add-kernels"
    open(out_file, "w").write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(kernels))


def main():
    if "--add-kernels" in sys.argv:
        return add_kernels(arg("--add-kernels", ""), arg("--out", ""))
    length, repeats, out_file = arg("--length", 1000000), arg("--repeats", 7), arg("--out", "")
    calls_only = "--calls-only" in sys.argv
    ctx = capi.Context(0)
    names, seqs, _ = synth.c3_workload(length)
    fasta = "".join(">%s\n%s\n" % (nm, seqs[nm]) for nm in names)
    t0 = time.time()
    text, _ = ctx.msa(fasta, synth.C3_NEWICK, workers=4)
    msa_s = time.time() - t0
    g, pnames = capi.read_gfa(text, add_sentinels=True)
    n = len(pnames)
    pairs45 = [(a, b) for a in range(n) for b in range(a + 1, n)]
    pairs1225 = [pairs45[k % len(pairs45)] for k in range(1225)]
    steps = [int(g.path_off[p + 1] - g.path_off[p]) for p in range(n)]
    out = {"workload": "configs[2] root graph, %d paths of %d-%d steps, %d nodes" % (n, min(steps), max(steps), len(g.label)), "msa_s": round(msa_s, 2),
           "repeats": repeats}
    capi.induced_pairwise_cigars(g, pairs45[:2], ctx)   # warm: code objects, the pool
    capi.induced_pairwise_stats(g, pairs45[:2], ctx)
    for tag, pairs in (("45", pairs45), ("1225", pairs1225)):
        stats_s, cigars_s, parse_s = [], [], []
        identical = True
        for _ in range(repeats if not calls_only else 1):
            t0 = time.time()
            st = capi.induced_pairwise_stats(g, pairs, ctx)
            stats_s.append(time.time() - t0)
            t0 = time.time()
            cig = capi.induced_pairwise_cigars(g, pairs, ctx)
            t1 = time.time()
            parsed = [parse(c) for c in cig]
            t2 = time.time()
            cigars_s.append(t1 - t0)
            parse_s.append(t2 - t1)
            identical = identical and st.tolist() == parsed
        yard = [c + p for c, p in zip(cigars_s, parse_s)]
        p2_steps = sum(steps[b] for a, b in pairs)
        firsts = sorted({a for a, b in pairs})
        table = len(firsts) * 4 * len(g.label) + sum(steps[a] for a in firsts) * 20
        rec = {"stats_s": [round(v, 4) for v in stats_s], "cigars_s": [round(v, 4) for v in cigars_s], "parse_s": [round(v, 4) for v in parse_s],
               "stats_median_s": round(statistics.median(stats_s), 4), "yardstick_median_s": round(statistics.median(yard), 4),
               "yardstick_spread_s": round(max(yard) - min(yard), 4), "cigars_median_s": round(statistics.median(cigars_s), 4),
               "identical": identical, "cigar_bytes": sum(len(c) for c in cig), "stats_bytes_back": 64 * len(pairs),
               # what the kernels must move at least: per path-2 step 4 B path node + 4 B table gather + 4 B emitted path-1 node + 2 label bytes (the
               # stats kernel once, the CIGAR kernels twice: count and write passes), plus each first path's table fill, scatter and check
               "bytes_min_stats": p2_steps * (4 + 4 + 4 + 2) + table, "bytes_min_cigars": 2 * p2_steps * (4 + 4 + 4 + 2) + table}
        rec["condition_stats_le_yardstick_plus_spread"] = rec["stats_median_s"] <= rec["yardstick_median_s"] + rec["yardstick_spread_s"]
        out["pairs_" + tag] = rec
    where = "one " + ctx.device_name()
    ctx.close()
    rec = {"what": "cl_induced_pairwise_stats (one device pass, 64 B back per pair) against the way to the same numbers without it: "
                   "cl_induced_pairwise_cigars, and that call plus a host parse of its text (Python re), on BASELINE configs[2]'s root graph "
                   "(10 x 1 Mbp, made by cl_msa in the same run); wall times of whole calls — graph upload, position tables, kernels, copy back — "
                   "that end in a device synchronise, alternating repeats in one process",
           "command": "python scripts/pair_stats_timing.py " + " ".join(sys.argv[1:]), "where": where,
           "condition": "stats median <= yardstick median + the yardstick's own spread (max - min over the repeats)", "timing": out}
    line = json.dumps(rec, indent=1)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        open(out_file, "w").write(line + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
