"""The -A output's cost (cl_msa -A / -c -A): the host loop (cl_induced_pairwise_cigar once per pair) against one device call
(cl_induced_pairwise_cigars) on the root graph of BASELINE configs[2] (10 x 1 Mbp, made by cl_msa in the same run), for its 45 pairs and for
the 45 repeated to 1 225 (configs[4]'s pair count at 1 Mbp); then the .maf stage (cl_induced_cyclic_maf over the host pool) on the 16 x 12 kbp
-c golden.  Prints one JSON line.

usage:  python scripts/induced_pairs_timing.py [--length 1000000] [--skip-host-1225]
Kernel times: run it once of its own under rocprofv3 --kernel-trace --stats.
"""
import gzip
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centrolign_amd import capi, synth  # noqa: E402


def host_loop(g, pairs):
    return [capi.induced_pairwise_cigar(g, a, b) for a, b in pairs]


def main():
    length = int(sys.argv[sys.argv.index("--length") + 1]) if "--length" in sys.argv else 1000000
    ctx = capi.Context(0)
    names, seqs, _ = synth.c3_workload(length)
    fasta = "".join(">%s\n%s\n" % (nm, seqs[nm]) for nm in names)
    t0 = time.time()
    text, st = ctx.msa(fasta, synth.C3_NEWICK, workers=4)
    msa_s = time.time() - t0
    g, pnames = capi.read_gfa(text, add_sentinels=True)
    n = len(pnames)
    pairs45 = [(a, b) for a in range(n) for b in range(a + 1, n)]
    pairs1225 = [pairs45[k % len(pairs45)] for k in range(1225)]
    steps = [int(g.path_off[p + 1] - g.path_off[p]) for p in range(n)]
    out = {"workload": "configs[2] root graph, %d paths of %d-%d steps, %d nodes" % (n, min(steps), max(steps), len(g.label)), "msa_s": round(msa_s, 2)}
    capi.induced_pairwise_cigars(g, pairs45[:2], ctx)   # warm: code objects, the pool
    for tag, pairs in (("45", pairs45), ("1225", pairs1225)):
        t0 = time.time()
        dev = capi.induced_pairwise_cigars(g, pairs, ctx)
        dev_s = time.time() - t0
        t0 = time.time()
        dev2 = capi.induced_pairwise_cigars(g, pairs, ctx)
        dev2_s = time.time() - t0
        rec = {"device_s": round(dev_s, 4), "device_again_s": round(dev2_s, 4), "cigar_bytes": sum(len(c) for c in dev)}
        if tag == "45" or "--skip-host-1225" not in sys.argv:
            t0 = time.time()
            host = host_loop(g, pairs)
            rec["host_loop_s"] = round(time.time() - t0, 3)
            rec["identical"] = host == dev == dev2
        # what the kernels must move at least: path 2 (4 B) + its gather (4 B) + the emitted path-1 node and two labels per step, twice (count and
        # write passes); the position table (fill 4 B, scatter 4 + 4 B, check 4 + 4 + 4 B per path-1 step) once per first path in the batch
        p2_steps = sum(steps[b] for a, b in pairs)
        firsts = sorted({a for a, b in pairs})
        rec["bytes_min"] = 2 * p2_steps * (4 + 4 + 4 + 2) + len(firsts) * 4 * len(g.label) + sum(steps[a] for a in firsts) * 20
        out["pairs_" + tag] = rec
    # the .maf stage at 16 x 12 kbp: the reference's cyclised graph, every pair, over the host threads
    cg, cn = capi.read_gfa(gzip.decompress(open(os.path.join(ROOT, "tests", "golden", "cyclize_16x12k.gfa.gz"), "rb").read()), add_sentinels=False)
    cpairs = [(a, b) for a in range(len(cn)) for b in range(a + 1, len(cn))]
    threads = min(32, os.cpu_count() or 1)
    t0 = time.time()
    for a, b in cpairs:
        capi.induced_cyclic_maf(cg, a, b, cn[a], cn[b])
    one_s = time.time() - t0
    t0 = time.time()
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda p: capi.induced_cyclic_maf(cg, p[0], p[1], cn[p[0]], cn[p[1]]), cpairs))
    out["maf_16x12k"] = {"pairs": len(cpairs), "one_thread_s": round(one_s, 3), "threads": threads, "threaded_s": round(time.time() - t0, 3)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
