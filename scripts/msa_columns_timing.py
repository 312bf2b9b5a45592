"""What the MSA as columns costs: cl_msa_columns_compute (device) and cl_msa_columns_host on the root graph of BASELINE configs[2] (10 x 1 Mbp
under its guide tree), made by cl_msa in the same run; both layouts, several times each in the same process, alternating, everything wanted.  Both
calls begin with the same host level pass (cl_msa_column_layout); its wall time inside each call (cl_msa_columns_layout_seconds) and its share
of the call are reported.  Wall times of
whole calls; the device call ends in a device synchronise.  Device-only kernel times are not measured.  No threshold: nothing computed a column MSA
before.  Writes one JSON record (--out FILE, default standard output).

usage:  python scripts/msa_columns_timing.py [--length 1000000] [--repeats 7] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from centrolign_amd import capi, synth  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def spread(values):
    return {"median_s": round(statistics.median(values), 4), "min_max_s": [round(min(values), 4), round(max(values), 4)], "all_s": [round(v, 4) for v in values]}


def main():
    length, repeats, out_file = arg("--length", 1000000), arg("--repeats", 7), arg("--out", "")
    ctx = capi.Context(0)
    names, seqs, _ = synth.c3_workload(length)
    fasta = "".join(">%s\n%s\n" % (nm, seqs[nm]) for nm in names)
    t0 = time.time()
    text, _ = ctx.msa(fasta, synth.C3_NEWICK, workers=4)
    msa_s = time.time() - t0
    g, path_names = capi.read_gfa(text, add_sentinels=True)
    n = len(path_names)
    steps = int(g.path_off[-1])
    out = {"workload": "configs[2]: %d paths, %d steps, %d nodes" % (n, steps, len(g.label)), "msa_s": round(msa_s, 2), "repeats": repeats}
    capi.msa_columns(g, ctx, want=7, block_cols=4096)   # warm: code objects, the pool
    times = {layout: {"device": [], "host": [], "level_in_device": [], "level_in_host": []} for layout in ("level", "node")}
    last = {}
    for _ in range(repeats):
        for layout in ("level", "node"):
            t0 = time.time()
            dev = capi.msa_columns(g, ctx, layout=layout)
            t1 = time.time()
            times[layout]["level_in_device"].append(capi.msa_columns_layout_seconds())
            t2 = time.time()
            host = capi.msa_columns_host(g, layout=layout)
            t3 = time.time()
            times[layout]["level_in_host"].append(capi.msa_columns_layout_seconds())
            times[layout]["device"].append(t1 - t0)
            times[layout]["host"].append(t3 - t2)
            last[layout] = (dev, host)
    for layout in ("level", "node"):
        dev, host = last[layout]
        W, S = dev["n_cols"], dev["n_sites"]
        rec = {"n_cols": W, "n_sites": S,
               "identical_to_host": all(np.array_equal(dev[k], host[k]) for k in ("node_col", "rows", "columns", "site_col", "site_rows")),
               "device": spread(times[layout]["device"]), "host": spread(times[layout]["host"]),
               "level_pass_in_device": spread(times[layout]["level_in_device"]), "level_pass_in_host": spread(times[layout]["level_in_host"]),
               "level_pass_share_of_device": round(statistics.median(times[layout]["level_in_device"]) / statistics.median(times[layout]["device"]), 3),
               "level_pass_share_of_host": round(statistics.median(times[layout]["level_in_host"]) / statistics.median(times[layout]["host"]), 3),
               "bytes_back": n * W + 32 * W + 8 * S + n * S,
               # what the device pass must move at least: the preset of the tile, per step 1 B stored and 4 B path node + 4 B column + 1 B label
               # read, the tile read once by the reduce, 32 B written per column (and read again by the two site passes: 2 x 4 B of flags)
               "bytes_min_device": n * W + steps * (1 + 9) + n * W + 32 * W + 8 * W}
        out[layout] = rec
    where = "one " + ctx.device_name().strip()
    ctx.close()
    rec = {"what": "cl_msa_columns_compute and cl_msa_columns_host with everything wanted (rows, column records, sites) on BASELINE configs[2]'s root "
                   "graph (made by cl_msa in the same run), both layouts; wall times of whole calls — the host level pass, the upload, the kernels "
                   "block by block, the copies back — alternating repeats in one process; level_pass_in_* is the wall time of the level pass inside the call "
                   "(cl_msa_columns_layout_seconds); device-only kernel times were not measured",
           "command": "python scripts/msa_columns_timing.py " + " ".join(sys.argv[1:]), "where": where, "condition": "none: reported as it comes out", "timing": out}
    line = json.dumps(rec, indent=1)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        open(out_file, "w").write(line + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
