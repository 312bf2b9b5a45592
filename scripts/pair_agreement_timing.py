"""What comparing two alignments costs: one cl_induced_pairwise_agreements call against the only way to the same numbers before it existed,
cl_induced_pairwise_cigars on graph a plus the same call on graph b — without the host parse those texts then need, so that no interpreter time
is measured.  Graph a is the root graph of BASELINE configs[2] (10 x 1 Mbp under its guide tree), graph b the graph of the same sequences under
the tree --infer-tree gives them, both made by cl_msa in the same run; the 45 pairs and the 45 repeated to 1 225, several times each in the same
process, alternating.  Wall times of whole calls, which end in a device synchronise.  Device-only kernel times are not measured.  Writes one JSON
record (--out FILE, default standard output).

usage:  python scripts/pair_agreement_timing.py [--length 1000000] [--repeats 7] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centrolign_amd import capi, synth  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    length, repeats, out_file = arg("--length", 1000000), arg("--repeats", 7), arg("--out", "")
    ctx = capi.Context(0)
    names, seqs, _ = synth.c3_workload(length)
    fasta = "".join(">%s\n%s\n" % (nm, seqs[nm]) for nm in names)
    t0 = time.time()
    text_a, _ = ctx.msa(fasta, synth.C3_NEWICK, workers=4)
    inferred = capi.infer_guide_tree(ctx, fasta)
    text_b, _ = ctx.msa(fasta, inferred, workers=4)
    msa_s = time.time() - t0
    a, names_a = capi.read_gfa(text_a, add_sentinels=True)
    b, names_b = capi.read_gfa(text_b, add_sentinels=True)
    n = len(names_a)
    in_b = [names_b.index(nm) for nm in names_a]
    pairs45 = [(p, q) for p in range(n) for q in range(p + 1, n)]
    quads45 = [(p, q, in_b[p], in_b[q]) for p, q in pairs45]
    quads1225 = [quads45[k % len(quads45)] for k in range(1225)]
    steps = [int(a.path_off[p + 1] - a.path_off[p]) for p in range(n)]
    out = {"workload": "configs[2]: %d paths of %d-%d steps; graph a under its guide tree (%d nodes), graph b under the inferred tree (%d nodes)"
                       % (n, min(steps), max(steps), len(a.label), len(b.label)),
           "inferred_tree": inferred if isinstance(inferred, str) else inferred.decode(), "same_tree": text_a == text_b, "msa_s": round(msa_s, 2), "repeats": repeats}
    capi.induced_pairwise_cigars(a, pairs45[:2], ctx)   # warm: code objects, the pool
    capi.induced_pairwise_agreements(a, b, quads45[:2], ctx)
    for tag, quads in (("45", quads45), ("1225", quads1225)):
        pairs_a, pairs_b = [qd[:2] for qd in quads], [qd[2:] for qd in quads]
        agreement_s, cigars_s = [], []
        for _ in range(repeats):
            t0 = time.time()
            got = capi.induced_pairwise_agreements(a, b, quads, ctx)
            t1 = time.time()
            cig_a = capi.induced_pairwise_cigars(a, pairs_a, ctx)
            cig_b = capi.induced_pairwise_cigars(b, pairs_b, ctx)
            t2 = time.time()
            agreement_s.append(t1 - t0)
            cigars_s.append(t2 - t1)
        # the last repeat's results against the host definition, on the distinct quads
        identical = all(got[k].tolist() == [capi.induced_pairwise_agreement(a, qd[0], qd[1], b, qd[2], qd[3])[f] for f in capi.PAIR_AGREEMENT_FIELDS]
                        for k, qd in enumerate(quads[:45]))
        p2_steps = sum(steps[qd[1]] for qd in quads)
        table = 0
        for g, firsts in ((a, sorted({qd[0] for qd in quads})), (b, sorted({qd[2] for qd in quads}))):
            table += len(firsts) * 4 * len(g.label) + sum(int(g.path_off[p + 1] - g.path_off[p]) for p in firsts) * 20
        shared, aligned_a, aligned_b = int(got[:, 2].sum()), int(got[:, 0].sum()), int(got[:, 1].sum())
        rec = {"agreement_s": [round(v, 4) for v in agreement_s], "cigars_s": [round(v, 4) for v in cigars_s],
               "agreement_median_s": round(statistics.median(agreement_s), 4), "agreement_min_max_s": [round(min(agreement_s), 4), round(max(agreement_s), 4)],
               "yardstick_median_s": round(statistics.median(cigars_s), 4), "yardstick_min_max_s": [round(min(cigars_s), 4), round(max(cigars_s), 4)],
               "yardstick_spread_s": round(max(cigars_s) - min(cigars_s), 4),
               "identical_to_host": identical, "recall": round(shared / max(aligned_a, 1), 6), "precision": round(shared / max(aligned_b, 1), 6),
               "agreement_bytes_back": 64 * len(quads), "cigar_bytes_back": sum(len(c) for c in cig_a) + sum(len(c) for c in cig_b),
               # what the kernels must move at least: per path-2 step and graph 4 B path node + 4 B table gather + 4 B emitted path-1 node + 2 label
               # bytes (what the statistics kernel reads), plus 4 B of partner word written and 4 B read, the 4 B of the preset, and each first
               # path's table fill, scatter and check; the CIGAR calls read the same twice per graph (count and write passes)
               "bytes_min_agreement": p2_steps * (2 * (4 + 4 + 4 + 2) + 4 + 4 + 4) + table, "bytes_min_cigars": 2 * 2 * p2_steps * (4 + 4 + 4 + 2) + table}
        rec["condition_agreement_le_yardstick_plus_spread"] = rec["agreement_median_s"] <= rec["yardstick_median_s"] + rec["yardstick_spread_s"]
        out["pairs_" + tag] = rec
    where = "one " + ctx.device_name().strip()   # (the marketing name can come back empty: the architecture string remains)
    ctx.close()
    rec = {"what": "cl_induced_pairwise_agreements (64 B back per quad) against the only earlier way to the same numbers, cl_induced_pairwise_cigars on "
                   "graph a plus the same call on graph b (the host parse left out), on BASELINE configs[2]'s root graph and the graph of the same "
                   "sequences under the inferred tree (both made by cl_msa in the same run); wall times of whole calls — both graphs' upload, position "
                   "tables, kernels, copy back — that end in a device synchronise, alternating repeats in one process; device-only kernel times were "
                   "not measured",
           "command": "python scripts/pair_agreement_timing.py " + " ".join(sys.argv[1:]), "where": where,
           "condition": "median of the new call <= yardstick median + the yardstick's own spread (max - min over the repeats)", "timing": out}
    line = json.dumps(rec, indent=1)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        open(out_file, "w").write(line + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
