"""Goldens for the CLI's -A output combined with -c (src/core.cpp:523-591): the PREFIX_<a>_<b>.txt CIGARs written from the acyclic root graph
before apply_bonds, and the PREFIX_<a>_<b>.maf blocks written from the cyclised and polished graph, as the UNMODIFIED compiled reference
(oracle/_ref/ref_cli) writes them.  Stored: the size and sha256 of every file, and the full text of a handful of .maf files (gzip).

  induced_16x12k   the inputs and parameters of make_cyclize_wide.py's cyclize_16x12k (bonds found: the .maf files come from a cyclic graph)
  induced_nobond   six point-mutated copies of one random 3 kbp sequence: no bond is found, and the reference still writes one .maf beside every .txt

The reference's -c text depends on its heap (it reads past a vector's end in Bonder::trim_partition_ends), and -A changes the
heap, so --perturb N runs it with glibc's MALLOC_PERTURB_=N: the fill byte under which its -c -A run prints the GFA the committed -c golden
holds (recorded in the JSON).

usage (build container only):  python tests/golden/make_induced_maf.py CASE [--perturb N]
"""
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CASES = {   # name: (sequences, names, newick, min_cyclizing_length, max_num_match_pairs, number of .maf texts kept whole)
    "induced_16x12k": None,   # make_cyclize_wide.CASES["cyclize_16x12k"]
    "induced_nobond": None,
    "induced_50x8k": None,    # make_cyclize_wide.CASES["cyclize_50x8k"]
}
KEEP = 6


def workload(case):
    from centrolign_amd import msa, synth
    if case in ("induced_16x12k", "induced_50x8k"):
        import make_cyclize_wide as mcw
        wide = case.replace("induced", "cyclize")
        names, seqs, newick = mcw.workload(wide)
        c = mcw.CASES[wide]
        return names, seqs, newick, c[6], c[7]
    if case == "induced_nobond":
        import random
        rng = random.Random(47)
        anc = [rng.choice("ACGT") for _ in range(3000)]
        seqs = ["".join(c if rng.random() > 0.01 else rng.choice("ACGT") for c in anc) for _ in range(6)]
        names = ["n%d" % i for i in range(6)]
        return names, seqs, msa.newick(msa.balanced_tree(names)) + ";", 1500, 20000
    raise KeyError(case)


def reference_outputs(d, names, seqs, newick, min_len, budget, perturb=None):
    """run ref_cli -c -A in d; {file name without the prefix: bytes}, and the GFA"""
    from centrolign_amd import synth
    synth.write_fasta(os.path.join(d, "in.fa"), seqs, names)
    open(os.path.join(d, "t.nwk"), "w").write(newick + "\n")
    subprocess.check_call(["bash", "-c", "cd %s && %s in.fa t.nwk - out.gfa 0 2 0 's:all_pairs_prefix=pw;b:cyclize_tandem_duplications=1;"
                           "i:min_cyclizing_length=%d;i:max_num_match_pairs=%d' > ref.log 2>&1"
                           % (d, os.path.join(ROOT, "oracle", "_ref", "ref_cli"), min_len, budget)],
                          env=dict(os.environ, **({"MALLOC_PERTURB_": str(perturb)} if perturb is not None else {})))
    files = {}
    for f in sorted(os.listdir(d)):
        if f.startswith("pw_") and (f.endswith(".txt") or f.endswith(".maf")):
            files[f[3:]] = open(os.path.join(d, f), "rb").read()
    return files, open(os.path.join(d, "out.gfa"), "rb").read()


def main():
    case = sys.argv[1]
    names, seqs, newick, min_len, budget = workload(case)
    perturb = int(sys.argv[sys.argv.index("--perturb") + 1]) if "--perturb" in sys.argv else None
    d = tempfile.mkdtemp(prefix="induced_ref_")
    files, gfa = reference_outputs(d, names, seqs, newick, min_len, budget, perturb)
    mafs = sorted(f for f in files if f.endswith(".maf"))
    keep = mafs[:: max(1, len(mafs) // KEEP)][:KEEP]
    out = {"names": names, "newick": newick, "min_cyclizing_length": min_len, "max_num_match_pairs": budget,
           "input_sha256": hashlib.sha256("".join(seqs).encode()).hexdigest(),
           "reference": "oracle/_ref/ref_cli -c -A (the unmodified reference)", "malloc_perturb": perturb,
           "gfa": {"sha256": hashlib.sha256(gfa).hexdigest(), "bytes": len(gfa)},
           "files": {f: {"sha256": hashlib.sha256(b).hexdigest(), "bytes": len(b)} for f, b in sorted(files.items())},
           "kept": keep}
    with open(os.path.join(HERE, case + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    if case == "induced_nobond":   # (the 16 x 12 kbp run prints the GFA of cyclize_16x12k.gfa.gz under its fill byte)
        with open(os.path.join(HERE, case + ".gfa.gz"), "wb") as f:
            f.write(gzip.compress(gfa, 9, mtime=0))
    with open(os.path.join(HERE, case + "_maf.json.gz"), "wb") as f:
        f.write(gzip.compress(json.dumps({k: files[k].decode() for k in keep}).encode(), 9, mtime=0))
    print(case, len(files), "files,", len(mafs), ".maf, GFA", len(gfa), "bytes")


if __name__ == "__main__":
    main()
