"""What the position-resolved outputs cost: one cl_induced_pairwise_profiles call (1 000-base windows) and one cl_induced_gap_events_batch call
(events of at least 50 bases) against the only way to positions before they existed, cl_induced_pairwise_cigars — without the host parse that
text then needs, so that no interpreter time is measured — on the root graph of BASELINE configs[2] (10 x 1 Mbp, made by cl_msa in the same run),
for its 45 pairs and for the 45 repeated to 1 225, several times each in the same process, alternating.  Wall times of whole calls, which end in
a device synchronise.  Device-only kernel times are not measured.  Writes one JSON record (--out FILE, default standard output).

usage:  python scripts/pair_profile_timing.py [--length 1000000] [--repeats 7] [--window 1000] [--min-event 50] [--out FILE]
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
    window, min_event = arg("--window", 1000), arg("--min-event", 50)
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
           "repeats": repeats, "window": window, "min_event": min_event}
    capi.induced_pairwise_cigars(g, pairs45[:2], ctx)   # warm: code objects, the pool
    capi.induced_pairwise_profiles(g, pairs45[:2], window, ctx)
    capi.induced_gap_events_batch(g, pairs45[:2], min_event, ctx)
    for tag, pairs in (("45", pairs45), ("1225", pairs1225)):
        profiles_s, events_s, cigars_s = [], [], []
        for _ in range(repeats):
            t0 = time.time()
            prof = capi.induced_pairwise_profiles(g, pairs, window, ctx)
            t1 = time.time()
            ev = capi.induced_gap_events_batch(g, pairs, min_event, ctx)
            t2 = time.time()
            cig = capi.induced_pairwise_cigars(g, pairs, ctx)
            t3 = time.time()
            profiles_s.append(t1 - t0)
            events_s.append(t2 - t1)
            cigars_s.append(t3 - t2)
        # the last repeat's results against the host definitions, on the distinct pairs
        identical = all(prof[k].tolist() == capi.induced_pairwise_profile(g, a, b, window).tolist()
                        and ev[k].tolist() == capi.induced_gap_events(g, a, b, min_event).tolist() for k, (a, b) in enumerate(pairs[:45]))
        p2_steps = sum(steps[b] for a, b in pairs)
        firsts = sorted({a for a, b in pairs})
        table = len(firsts) * 4 * len(g.label) + sum(steps[a] for a in firsts) * 20
        spread = max(cigars_s) - min(cigars_s)
        rec = {"profiles_s": [round(v, 4) for v in profiles_s], "events_s": [round(v, 4) for v in events_s], "cigars_s": [round(v, 4) for v in cigars_s],
               "profiles_median_s": round(statistics.median(profiles_s), 4), "profiles_spread_s": round(max(profiles_s) - min(profiles_s), 4),
               "events_median_s": round(statistics.median(events_s), 4), "events_spread_s": round(max(events_s) - min(events_s), 4),
               "yardstick_median_s": round(statistics.median(cigars_s), 4), "yardstick_spread_s": round(spread, 4),
               "identical_to_host": identical, "cigar_bytes": sum(len(c) for c in cig),
               "profile_bytes_back": 32 * sum(len(p) for p in prof), "event_bytes_back": 32 * sum(len(e) for e in ev),
               # what the kernels must read at least: per path-2 step 4 B path node + 4 B table gather + 4 B emitted path-1 node + 2 label bytes (the
               # profile kernel once; the events and CIGAR kernels twice: count and write passes), plus each first path's table fill, scatter and check
               "bytes_min_profiles": p2_steps * (4 + 4 + 4 + 2) + table, "bytes_min_events": 2 * p2_steps * (4 + 4 + 4 + 2) + table,
               "bytes_min_cigars": 2 * p2_steps * (4 + 4 + 4 + 2) + table}
        rec["condition_profiles_le_yardstick_plus_spread"] = rec["profiles_median_s"] <= rec["yardstick_median_s"] + rec["yardstick_spread_s"]
        rec["condition_events_le_yardstick_plus_spread"] = rec["events_median_s"] <= rec["yardstick_median_s"] + rec["yardstick_spread_s"]
        out["pairs_" + tag] = rec
    where = "one " + ctx.device_name()
    ctx.close()
    rec = {"what": "cl_induced_pairwise_profiles (32 B back per window) and cl_induced_gap_events_batch (32 B back per event) against the only earlier "
                   "way to positions, cl_induced_pairwise_cigars (its host parse left out), on BASELINE configs[2]'s root graph (10 x 1 Mbp, made by "
                   "cl_msa in the same run); wall times of whole calls — graph upload, position tables, kernels, copy back — that end in a device "
                   "synchronise, alternating repeats in one process; device-only kernel times were not measured",
           "command": "python scripts/pair_profile_timing.py " + " ".join(sys.argv[1:]), "where": where,
           "condition": "median of each new call <= yardstick median + the yardstick's own spread (max - min over the repeats)", "timing": out}
    line = json.dumps(rec, indent=1)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        open(out_file, "w").write(line + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
