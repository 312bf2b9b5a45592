"""Does a guide tree rebuilt from alignment distances (cl_refine_guide_tree, the CLI's --refine-tree) come closer to the truth than the k-mer tree
(--infer-tree) or the FASTA order it started from?  Simulated families with a known tree — eight leaves, ((((0,1),(2,3)),((4,5),(6,7))), evolved
from one HOR array as tests/test_gpu_tree_infer.evolve_family does, written to the FASTA in a shuffled order — at several seeds.  Per seed and start
(FASTA order; k-mer tree): the Robinson-Foulds distance to the true tree (bipartitions in one tree and not the other) of the start and after one
and two refinement rounds, and the wall time of each.  Writes one JSON record (--out FILE, default standard output).

usage:  python scripts/refine_tree_eval.py [--seeds 3,4,5] [--length 100000] [--budget 1250000] [--out FILE]
"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from centrolign_amd import capi, synth  # noqa: E402

TRUE_TREE = "(((leaf0,leaf1),(leaf2,leaf3)),((leaf4,leaf5),(leaf6,leaf7)));"   # five internal edges once unrooted


def evolve_family(seed, length):
    rng = random.Random(seed)
    root = synth.hor_sequences(seed, length, 1)[0]

    def down(s, r):
        return "".join(synth._mut_track(rng, s, r)[0])

    leaves = []
    for a in (down(root, 0.003), down(root, 0.003)):
        for b in (down(a, 0.003), down(a, 0.003)):
            leaves += [down(b, 0.002), down(b, 0.002)]
    return leaves


def leaf_sets(newick):
    """the leaf set under every internal node of a Newick text with quoted or bare labels"""
    sets, stack, i = [], [], 0
    while i < len(newick):
        c = newick[i]
        if c == "(":
            stack.append(set())
            i += 1
        elif c == ")":
            done = stack.pop()
            sets.append(frozenset(done))
            if stack:
                stack[-1] |= done
            i += 1
        elif c in ",;":
            i += 1
        elif c == ":":
            while i < len(newick) and newick[i] not in ",);":
                i += 1
        else:
            j = newick.index('"', i + 1) + 1 if c == '"' else min(k for k in range(i, len(newick) + 1) if k == len(newick) or newick[k] in ":,);")
            stack[-1].add(newick[i:j].strip('"'))
            i = j
    return sets


def splits(newick, names):
    """the non-trivial bipartitions, each as its side without names[0]"""
    everyone = frozenset(names)
    out = set()
    for s in leaf_sets(newick):
        side = everyone - s if names[0] in s else s
        if 2 <= len(side) <= len(names) - 2:
            out.add(frozenset(side))
    return out


def in_order_newick(names):
    """the tree cl_msa takes when none is given: the sequences joined one after the other in FASTA order"""
    t = names[0]
    for nm in names[1:]:
        t = "(%s,%s)" % (t, nm)
    return t + ";"


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    seeds = [int(s) for s in arg("--seeds", "3,4,5").split(",")]
    length, budget, out_file = arg("--length", 100000), arg("--budget", 1250000), arg("--out", "")
    ctx = capi.Context(0)
    rows = []
    for seed in seeds:
        leaves = evolve_family(seed, length)
        order = list(range(8))
        random.Random(1000 + seed).shuffle(order)
        names = ["leaf%d" % i for i in order]
        fasta = "".join(">%s\n%s\n" % (nm, leaves[i]) for nm, i in zip(names, order))
        truth = splits(TRUE_TREE, names)
        assert len(truth) == 5

        def rf(newick):
            return len(splits(newick, names) ^ truth)

        t0 = time.time()
        kmer_tree = capi.infer_guide_tree(ctx, fasta)
        kmer_s = time.time() - t0
        rec = {"seed": seed, "fasta_names": names, "length": length}
        for tag, start, start_text, start_s in (("fasta_order", None, in_order_newick(names), 0.0), ("kmer_tree", kmer_tree, kmer_tree, kmer_s)):
            r = {"rf_start": rf(start_text), "start_s": round(start_s, 3)}
            for rounds in (1, 2):
                t0 = time.time()
                tree, run, conv = ctx.refine_guide_tree(fasta, start, rounds, max_num_match_pairs=budget)
                r["rf_refine_%d" % rounds] = rf(tree)
                r["refine_%d_s" % rounds] = round(time.time() - t0, 3)
                r["refine_%d_rounds_run" % rounds], r["refine_%d_converged" % rounds] = run, conv
            rec[tag] = r
        rows.append(rec)
        print(json.dumps(rec), file=sys.stderr)
    ctx.close()
    line = json.dumps({"what": "Robinson-Foulds distance to the true tree (bipartitions in one tree and not the other; 0-10 for eight leaves) of the "
                               "FASTA-order start and of the --infer-tree tree, each as it is and after --refine-tree 1 and 2 (cl_refine_guide_tree), and the "
                               "wall time of each; eight leaves evolved from one HOR array along " + TRUE_TREE + ", FASTA order shuffled (fasta_names)",
                       "command": "python scripts/refine_tree_eval.py " + " ".join(sys.argv[1:]), "workers": 1, "rows": rows}, indent=1)
    if out_file:
        os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
        open(out_file, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
