"""centrolign_amd/bin/centrolign end to end on the device: the reference's command line in, the reference's output text and files out
(the goldens of test_msa.py, test_gpu_subalignments.py and test_gpu_induced_pairs.py, reached through the executable instead of cl_msa's
ctypes binding).  Every run is one fresh child process with its own time limit, one at a time; after a child that ends by a signal or
times out, no further child is started in this module."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from centrolign_amd import msa, synth
from tests import helpers as H
from tests.golden import make_induced_maf as mim
from tests.golden import make_subalignments as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
Z = np.load(os.path.join(H.GOLDEN, "msa_text.npz"))
SUB = json.load(open(os.path.join(H.GOLDEN, "subalignments.json")))
_faulted = []


def run(args, cwd, timeout=900):
    if _faulted:
        pytest.fail("an earlier child of this module ended abnormally (%s): no further GPU process is started" % _faulted[0])
    try:
        r = subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired:
        _faulted.append("time limit of %d s" % timeout)
        raise
    if r.returncode < 0:
        _faulted.append("signal %d" % -r.returncode)
        pytest.fail("killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


def sha(b):
    return hashlib.sha256(b).hexdigest()


def write_inputs(d, names, seqs, newick, wrap=None):
    fa = "".join(">%s\n%s\n" % (nm, "\n".join(s[i:i + wrap] for i in range(0, len(s), wrap)) if wrap else s) for nm, s in zip(names, seqs))
    (d / "in.fa").write_text(fa)
    (d / "t.nwk").write_text(newick + "\n")
    return d / "in.fa", d / "t.nwk"


def msa_case(d, case):
    """the FASTA (80 columns) and Newick test_msa.py builds for a case of msa_text.npz"""
    name, n, length, seed, budget = case
    seqs = synth.hor_sequences(seed, length, n, seq_div=0.01, hor_div=0.03, indel_hor=2)
    names = ["seq%d" % i for i in range(n)]
    fa, nwk = write_inputs(d, names, seqs, msa.newick(msa.balanced_tree(names)) + ";", wrap=80)
    return fa, nwk, budget, bytes(Z[name])


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("case", H.msa_cases(), ids=lambda c: c[0])
def test_gpu_cli_plain_outputs(tmp_path, case, threads):
    """the CIGAR line (pairs) or the GFA (more sequences) the reference printed, byte for byte, with one and with three worker contexts"""
    fa, nwk, budget, want = msa_case(tmp_path, case)
    r = run(["-T", nwk, "-a", budget, "-t", threads, "-v", "0", fa], tmp_path)
    assert r.stdout == want and r.stderr == b""


@pytest.mark.gpu
def test_gpu_cli_from_a_config_file(tmp_path):
    """the same run with every parameter from a config file: the reference's default config with the inputs and the budget edited in"""
    case = [c for c in H.msa_cases() if c[0] == "msa4_8k"][0]
    fa, nwk, budget, want = msa_case(tmp_path, case)
    text = open(os.path.join(H.GOLDEN, "reference_default_config.txt")).read()
    for key, old, new in (("fasta_name", '""', str(fa)), ("tree_name", '""', str(nwk)), ("max_num_match_pairs", "1250000", str(budget)),
                          ("logging_level", "2", "1")):
        assert text.count(" %s: %s\n" % (key, old)) == 1
        text = text.replace(" %s: %s\n" % (key, old), " %s: %s\n" % (key, new))
    (tmp_path / "run.yaml").write_text(text)
    r = run(["-C", tmp_path / "run.yaml"], tmp_path)
    assert r.stdout == want
    assert b"warning" not in r.stderr and b"Run completed successfully" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [1, 3])
def test_gpu_cli_away_from_the_default_scoring(tmp_path, threads):
    """the one end-to-end run under non-default scoring (tests/golden/params_msa4_8k.yaml: stitch 3 / 4 / 2,9,30 / 5,2,1, anchor gaps 0,10,10 / 0.5,0.5,0, score function 1,
    count power 0.75), where host routes, partitioning and calibration see it together with the kernels: the GFA and the -s subalignment text of the compiled
    reference (tests/golden/make_golden.py msa_params), byte for byte, with one and with three worker contexts.  (On this input the reference's GFA under this
    config is the GFA under the default scoring: the case shows that the library follows the reference there, not that the scoring moves the result.)"""
    import gzip
    case = [c for c in H.msa_cases() if c[0] == "msa4_8k"][0]
    fa, nwk, budget, _ = msa_case(tmp_path, case)
    text = open(os.path.join(H.GOLDEN, "params_msa4_8k.yaml")).read()
    for key, old, new in (("fasta_name", '""', str(fa)), ("tree_name", '""', str(nwk)), ("max_num_match_pairs", "1250000", str(budget)),
                          ("subalignments_filepath", '""', str(tmp_path / "sub.txt")), ("threads", "1", str(threads)), ("logging_level", "2", "1")):
        assert text.count(" %s: %s\n" % (key, old)) == 1, key
        text = text.replace(" %s: %s\n" % (key, old), " %s: %s\n" % (key, new))
    (tmp_path / "run.yaml").write_text(text)
    r = run(["-C", tmp_path / "run.yaml"], tmp_path)
    want = gzip.open(os.path.join(H.GOLDEN, "params_msa4_8k.gfa.gz")).read()
    assert r.stdout == want
    assert (tmp_path / "sub.txt").read_bytes() == gzip.open(os.path.join(H.GOLDEN, "params_msa4_8k.sub.txt.gz")).read()
    assert b"warning" not in r.stderr


@pytest.mark.gpu
def test_gpu_cli_force_gfa_output(tmp_path):
    """two sequences: the root GFA with --force-gfa-output (the reference's root -S file), the CIGAR without"""
    from tests.test_gpu_subalignments import json_text
    names, seqs, newick, budget, _ = ms.workload("sub_two")
    fa, nwk = write_inputs(tmp_path, names, seqs, newick)
    r = run(["-T", nwk, "-a", budget, "--force-gfa-output", fa], tmp_path)
    assert r.stdout == json_text("sub_two", "root.gfa") and r.stdout.startswith(b"H\t")
    r = run(["-T", nwk, "-a", budget, fa], tmp_path)
    assert r.stdout == json_text("sub_two", "cigar.txt")


@pytest.mark.gpu
def test_gpu_cli_cyclize_and_all_pairs(tmp_path):
    """-c -y with the parameters cyclize_16x12k.json records: the reference's GFA; -A in the same run: every .txt and .maf file of
    induced_16x12k.json"""
    gold = json.load(open(os.path.join(H.GOLDEN, "cyclize_16x12k.json")))
    want = json.load(open(os.path.join(H.GOLDEN, "induced_16x12k.json")))
    names, seqs, newick, min_len, budget = mim.workload("induced_16x12k")
    assert newick == gold["newick"] and (min_len, budget) == (gold["min_cyclizing_length"], gold["max_num_match_pairs"])
    assert sha("".join(seqs).encode()) == gold["input_sha256"]
    fa, nwk = write_inputs(tmp_path, names, seqs, newick)
    out = tmp_path / "out"
    out.mkdir()
    r = run(["-T", nwk, "-c", "-y", min_len, "-a", budget, "-A", out / "pw", "-t", 3, fa], tmp_path, timeout=1200)
    assert sha(r.stdout) == gold["gfa"]["sha256"] and len(r.stdout) == gold["gfa"]["bytes"]
    files = {f[3:]: (out / f).read_bytes() for f in os.listdir(out)}
    assert sorted(files) == sorted(want["files"])
    for f, b in sorted(files.items()):
        assert sha(b) == want["files"][f]["sha256"], f


@pytest.mark.gpu
def test_gpu_cli_subalignments_file(tmp_path):
    """-s: the reference's subalignment file; a second run onto the same file refuses to start"""
    names, seqs, newick, budget, _ = ms.workload("sub_nobond")
    fa, nwk = write_inputs(tmp_path, names, seqs, newick)
    r = run(["-T", nwk, "-a", budget, "-s", tmp_path / "sub.txt", fa], tmp_path)
    assert sha((tmp_path / "sub.txt").read_bytes()) == SUB["sub_nobond"]["files"]["sub.txt"]["sha256"]
    if _faulted:
        pytest.fail("an earlier child of this module ended abnormally")
    again = subprocess.run([BIN, "-T", str(nwk), "-a", str(budget), "-s", str(tmp_path / "sub.txt"), str(fa)], cwd=str(tmp_path),
                           capture_output=True, timeout=300, stdin=subprocess.DEVNULL)
    assert again.returncode == 1 and again.stdout == b""
    assert ("error: Subalignment file already exists: %s" % (tmp_path / "sub.txt")) in again.stderr.decode()
    assert r.stdout  # the first run's GFA


@pytest.mark.gpu
def test_gpu_cli_restart(tmp_path):
    """-S, then -R in a second run after two subproblem files are gone: the same text, the loaded subproblems reported, and -s holds only
    the recomputed merges (the reference's file)"""
    names, seqs, newick, budget, _ = ms.workload("sub_restart")
    fa, nwk = write_inputs(tmp_path, names, seqs, newick)
    prefix = tmp_path / "sp"
    first = run(["-T", nwk, "-a", budget, "-S", prefix, fa], tmp_path)
    info = [ln.split("\t") for ln in open(str(prefix) + "_info.txt").read().split("\n")[1:] if ln]
    removed = {tuple(r) for r in SUB["sub_restart"]["removed"]}
    gone = [f for f, s in info if tuple(s.split(",")) in removed]
    assert len(gone) == 2
    for f in gone:
        os.remove(f)
    second = run(["-T", nwk, "-a", budget, "-S", prefix, "-R", "-s", tmp_path / "sub.txt", fa], tmp_path)
    assert second.stdout == first.stdout
    loaded = [ln for ln in second.stderr.decode().split("\n") if "subproblem(s) from an earlier run" in ln]
    assert len(loaded) == 1 and int(loaded[0].split("Loaded ")[1].split()[0]) > 0
    assert sha((tmp_path / "sub.txt").read_bytes()) == SUB["sub_restart"]["files"]["sub.txt"]["sha256"]


@pytest.mark.gpu
def test_gpu_cli_all_outputs_in_one_run(tmp_path):
    """one run that asks for the dot plot, the period spectra with their histogram, the monomer decomposition with its summary, the pair
    statistics and the aligned FASTA at once: its files and its standard output are, byte for byte, those of runs that ask for each alone
    (the --X-only runs for the three outputs that read the sequences).  Three sequences of about 3 kb under a balanced tree"""
    names = ["seq%d" % i for i in range(3)]
    seqs = synth.hor_sequences(11, 3000, 3, seq_div=0.01, hor_div=0.03, indel_hor=0)
    one = tmp_path / "one"
    one.mkdir()
    fa, nwk = write_inputs(one, names, seqs, msa.newick(msa.balanced_tree(names)) + ";", wrap=80)
    asked = {"dotplot": (["--dotplot", "dp.tsv"], ["dp.tsv"]),
             "periods": (["--periods", "pe.tsv", "--periods-hist", "ph.tsv"], ["pe.tsv", "ph.tsv"]),
             "monomers": (["--monomers", "mo.tsv", "--monomers-seed-period", 171, "--monomers-summary", "ms.tsv"], ["mo.tsv", "ms.tsv"]),
             "pair-stats": (["--pair-stats", "ps.tsv"], ["ps.tsv"]),
             "msa-out": (["--msa-out", "msa.fa"], ["msa.fa"])}
    together = run(["-T", nwk, "-v", 0] + [a for args, _ in asked.values() for a in args] + [fa], one, timeout=120)
    assert together.stdout.startswith(b"H\t") and together.stderr == b""
    assert sorted(os.listdir(one)) == sorted(["in.fa", "t.nwk"] + [f for _, made in asked.values() for f in made])
    for what, (args, made) in asked.items():
        d = tmp_path / what
        d.mkdir()
        alone = what in ("pair-stats", "msa-out")   # the others have an --X-only run: nothing is aligned or printed
        r = run((["-T", nwk] if alone else []) + ["-v", 0] + args + ([] if alone else ["--%s-only" % what]) + [fa], d, timeout=120)
        assert r.stdout == (together.stdout if alone else b"") and r.stderr == b"", what
        assert sorted(os.listdir(d)) == sorted(made), what
        for f in made:
            assert (d / f).read_bytes() == (one / f).read_bytes() and (d / f).stat().st_size > 0, (what, f)
