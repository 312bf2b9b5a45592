"""The -s output's cost at BASELINE configs[2] (10 x 1 Mbp, balanced tree, 4 workers):
  1. cl_msa with -S, without and with -s: wall time, the -s file's size, the GFA's sha256 (must not change), and the time to write the same
     bytes to a fresh file of the same file system (the part of the -s overhead that is the file system, not text production);
  2. the root merge's block alone: its two children read back from the -S files, cl_merge for the alignment, then cl_subalignment_text on the
     device against a host loop on one thread over the same data (numpy for the step table, the lines in a Python loop), bytes compared.
Prints one JSON line; --out FILE also writes it there.

usage:  python scripts/subalignment_timing.py [--length 1000000] [--out profiles/subalignment_timing.json]
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centrolign_amd import capi, synth  # noqa: E402

GAP = 2 ** 64 - 1


def host_block(g1, pn1, set1, g2, pn2, set2, pairs):
    """Core::emit_subalignment on one host thread"""
    def sides(g, names):
        n_paths = len(g.path_off) - 1
        path_of = np.repeat(np.arange(n_paths), np.diff(g.path_off.astype(np.int64)))
        step = np.arange(len(g.path_nodes)) - g.path_off[:-1].astype(np.int64)[path_of]
        nodes, first = np.unique(g.path_nodes, return_index=True)   # the first occurrence in (path, step) order
        out = {}
        dec = "ACGTN"
        for v, i in zip(nodes.tolist(), first.tolist()):
            lab = int(g.label[v])
            out[v] = "%s\t%d\t%s" % (names[path_of[i]], step[i], dec[lab] if lab < 5 else "\0")
        return out
    s1, s2 = sides(g1, pn1), sides(g2, pn2)
    gap = "-\t-\t-"
    head = "# sequence set 1\n" + "".join(s + "\n" for s in set1) + "# sequence set 2\n" + "".join(s + "\n" for s in set2) + "# alignment\n"
    body = "".join((gap if a == GAP else s1[a]) + "\t" + (gap if b == GAP else s2[b]) + "\n" for a, b in pairs.tolist())
    return (head + body).encode()


def main():
    length = int(sys.argv[sys.argv.index("--length") + 1]) if "--length" in sys.argv else 1000000
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    ctx = capi.Context(0)
    names, seqs, _ = synth.c3_workload(length)
    fasta = "".join(">%s\n%s\n" % (nm, seqs[nm]) for nm in names)
    d = tempfile.mkdtemp(prefix="subaln_timing_")
    res = {}
    wn, ws, _ = synth.c3_workload(20000)
    ctx.msa("".join(">%s\n%s\n" % (nm, ws[nm]) for nm in wn), synth.C3_NEWICK, workers=4)   # warm: code objects, pools, worker contexts
    try:
        runs = {}
        for tag in ("without_s", "with_s"):
            sub = os.path.join(d, "sub.txt")
            pre = os.path.join(d, tag, "sp")
            os.makedirs(os.path.dirname(pre))
            t0 = time.time()
            text, st = ctx.msa(fasta, synth.C3_NEWICK, workers=4, subproblems_prefix=pre, subalignments_path=sub if tag == "with_s" else None)
            runs[tag] = {"wall_s": round(time.time() - t0, 3), "gfa_sha256": hashlib.sha256(text).hexdigest(), "merges": int(st["n_merges"])}
            if tag == "with_s":
                data = open(sub, "rb").read()
                runs[tag]["s_bytes"] = len(data)
                runs[tag]["s_lines"] = data.count(b"\n")
                t0 = time.time()
                with open(os.path.join(d, "rewrite.txt"), "wb") as f:
                    f.write(data)
                runs[tag]["fs_write_same_bytes_s"] = round(time.time() - t0, 3)
                del data
        runs["s_overhead_s"] = round(runs["with_s"]["wall_s"] - runs["without_s"]["wall_s"], 3)
        runs["gfa_unchanged"] = runs["with_s"]["gfa_sha256"] == runs["without_s"]["gfa_sha256"]
        res["msa_4_workers"] = runs
        # the root merge's two children, as the run wrote them
        pre = os.path.join(d, "without_s", "sp")
        info = [ln.split("\t") for ln in open(pre + "_info.txt").read().split("\n")[1:] if ln]
        leaves, merges = capi.msa_plan(synth.C3_NEWICK, names)
        sets = [[names[s]] for s in leaves]
        for a, b in merges:
            sets.append(sets[a] + sets[b])
        a, b = merges[-1]
        graphs = []
        for slot in (a, b):
            f = [fn for fn, s in info if s == ",".join(sorted(sets[slot]))][0]
            graphs.append(capi.read_gfa(open(f, "rb").read(), add_sentinels=True))   # (path names in the graph's path order)
        (g1, pn1), (g2, pn2) = graphs
        m = ctx.merge(g1, g2, score_scale=float(st["score_scale"]))
        pairs = np.ascontiguousarray(m["alignment"], np.uint64)
        set1, set2 = sets[a][::-1], sets[b][::-1]
        capi.subalignment_text(ctx, g1, pn1, set1, g2, pn2, set2, pairs[:1000])   # warm: code objects, the pool
        times = []
        for _ in range(3):
            t0 = time.time()
            dev = capi.subalignment_text(ctx, g1, pn1, set1, g2, pn2, set2, pairs)
            times.append(round(time.time() - t0, 4))
        t0 = time.time()
        host = host_block(g1, pn1, set1, g2, pn2, set2, pairs)
        host_s = round(time.time() - t0, 3)
        steps = int(g1.path_off[-1] + g2.path_off[-1])
        res["root_block"] = {"paths": [len(pn1), len(pn2)], "path_steps": steps, "pairs": len(pairs), "bytes": len(dev), "device_s": times,
                             "host_one_thread_s": host_s, "identical": dev == host,
                             "device_GB_per_s_text": round(len(dev) / min(times) / 1e9, 2)}
    finally:
        shutil.rmtree(d, ignore_errors=True)
        ctx.close()
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
