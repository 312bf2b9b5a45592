"""The control plane without a device: centrolign_amd/bin/centrolign's options and config files, and the cl_config_* calls behind them
(cl_config_api.cpp).  The reference's own default config (tests/golden/reference_default_config.txt, its `centrolign -G`) is the
yardstick for keys, order and value formatting."""
import ctypes as C
import os
import subprocess

import pytest

from centrolign_amd import capi
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
FIXTURE = os.path.join(H.GOLDEN, "reference_default_config.txt")


def run(args, cwd=None, timeout=60):
    """one fresh child process with a time limit; a signal (a crash, an abort) fails the test on the spot"""
    r = subprocess.run([BIN] + list(args), cwd=cwd, capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    assert r.returncode >= 0, "killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace"))
    return r


def settings(text):
    """the non-comment lines of a config text"""
    return [ln for ln in text.split("\n") if not ln.lstrip().startswith("#")]


def values(text):
    out = {}
    for ln in settings(text):
        if ":" in ln:
            k, v = ln.split(":", 1)
            out[k.strip()] = v.strip()
    return out


def fixture_text():
    return open(FIXTURE).read()


def test_generated_config_is_the_references():
    r = run(["-G"])
    assert r.returncode == 0 and r.stderr == b""
    assert settings(r.stdout.decode()) == settings(fixture_text())
    keys = list(values(fixture_text()))
    assert len(keys) == 64 and list(values(r.stdout.decode())) == keys


def test_options_change_exactly_their_parameters():
    base = values(run(["-G"]).stdout.decode())
    got = values(run(["-m", "50", "-a", "1000", "-c", "-y", "5000", "-u", "-G"]).stdout.decode())
    assert {k: v for k, v in got.items() if base[k] != v} == {
        "max_count": "50", "max_num_match_pairs": "1000", "cyclize_tandem_duplications": "true", "min_cyclizing_length": "5000",
        "constraint_method": "0"}
    got = values(run(["-T", "t.nwk", "-A", "pw", "-S", "sp", "-s", "sub.txt", "-p", "0.25", "-g", "1", "-v", "3", "-R", "-t", "4",
                      "--skip-calibration", "--bond-prefix", "bd", "--force-gfa-output", "--devices", "0,0", "in.fa", "-G"]).stdout.decode())
    assert {k: v for k, v in got.items() if base[k] != v} == {
        "tree_name": "t.nwk", "all_pairs_prefix": "pw", "subproblems_prefix": "sp", "subalignments_filepath": "sub.txt",
        "pair_count_power": "0.25", "chaining_algorithm": "1", "logging_level": "3", "restart": "true", "threads": "4",
        "skip_calibration": "true", "bonds_prefix": "bd", "fasta_name": "in.fa"}
    # -p takes a decimal number; an integer is one too (the reference aborts on both)
    assert values(run(["-p", "2", "-G"]).stdout.decode())["pair_count_power"] == "2"


def test_generate_comes_before_the_config_file(tmp_path):
    cfg = tmp_path / "c.yaml"
    cfg.write_text("max_count: 77\n")
    r = run(["-C", str(cfg), "-G"])
    assert r.returncode == 0 and values(r.stdout.decode())["max_count"] == "3000"


def test_parsing_the_fixture_gives_the_defaults():
    assert capi.Config(fixture_text()).generate() == capi.Config().generate()
    assert settings(capi.Config().generate()) == settings(fixture_text())


def test_parse_generate_parse_round_trips():
    c = capi.Config()
    c["fasta_name"] = "my sequences.fa"         # whitespace: quoted
    c["tree_name"] = ""                         # empty: quoted
    c["subproblems_prefix"] = "out/sp"
    c["max_count"] = 17
    c["pair_count_power"] = 0.123456789012345   # more digits than 6: written so that it reads back the same
    c["window_length"] = 1e-300
    c["anchor_gap_open"] = (0.5, 60, 7000.25)
    c["stitch_gap_extend"] = (40, 6, 2)
    c["cyclize_tandem_duplications"] = True
    c["logging_level"] = 0
    text = c.generate()
    v = values(text)
    assert v["fasta_name"] == '"my sequences.fa"' and v["tree_name"] == '""' and v["subproblems_prefix"] == "out/sp"
    assert v["anchor_gap_open"] == "0.5,60,7000.25" and v["stitch_gap_extend"] == "40,6,2"
    back = capi.Config(text)
    assert back.generate() == text
    assert back["fasta_name"] == "my sequences.fa" and back["tree_name"] == "" and float(back["pair_count_power"]) == 0.123456789012345
    assert float(back["window_length"]) == 1e-300
    # the reader's conveniences: text before "---" is skipped, comments anywhere, quotes, spaces around the colon, T / F booleans
    other = capi.Config('preamble: is skipped\n---\n# comment\n  max_count :  17 # trailing\nfasta_name: "my sequences.fa"\n'
                        'tree_name: ""\nsubproblems_prefix: out/sp\npair_count_power: 0.123456789012345\nwindow_length: 1e-300\n'
                        'anchor_gap_open: 0.5,60,7000.25\nstitch_gap_extend: 40,6,2\ncyclize_tandem_duplications: T\nlogging_level: 0')
    assert other.generate() == text


@pytest.mark.parametrize("text,message", [
    ("max_count 5\n", "missing ':'"),
    ("no_such_parameter: 5\n", "No parameter with name no_such_parameter"),
    ("max_count: five\n", 'Could not parse "five" as an integer'),
    ("max_count: 5.5\n", 'Could not parse "5.5" as an integer'),
    ("restart: maybe\n", 'Could not parse "maybe" as a Boolean value'),
    ("window_length: wide\n", 'Could not parse "wide" as a decimal number'),
    ("anchor_gap_open: 1,2\n", "Expected 3 comma-separated values"),
    ("fasta_name: \"x\n", "Unmatched \""),
    (": 5\n", "no variable name"),
    ("max_count:\n", "no variable value"),
])
def test_config_errors(tmp_path, text, message):
    with pytest.raises(capi.ClError) as e:
        capi.Config(text)
    assert message in str(e.value)
    cfg = tmp_path / "bad.yaml"
    cfg.write_text(text)
    r = run(["-C", str(cfg)])
    assert r.returncode == 1 and r.stderr.decode().startswith("error: ") and message in r.stderr.decode()


@pytest.mark.parametrize("args,message", [
    (["-m", "0", "in.fa"], "Invalid value for parameter 'max_count', got 0 but expected a value > 0"),
    (["-p", "0", "in.fa"], "Invalid value for parameter 'pair_count_power'"),
    (["-v", "5", "in.fa"], "Invalid value for parameter 'logging_level', got 5 but expected a value <= 4"),
    (["-g", "3", "in.fa"], "Invalid value for parameter 'chaining_algorithm'"),
    (["-t", "0", "in.fa"], "Invalid value for parameter 'threads'"),
    (["-R", "in.fa"], "Cannot restart mid-execution without setting 'subproblems_prefix'"),
    ([], "FASTA input is missing"),
    (["-m", "many", "in.fa"], 'Could not parse "many" as an integer'),
    (["-p", "x", "in.fa"], 'Could not parse "x" as a decimal number'),
    (["--bogus", "in.fa"], "unknown option '--bogus'"),
    (["-Z", "in.fa"], "unknown option '-Z'"),
    (["in.fa", "-T"], "requires an argument"),
    (["--devices", "0,x", "in.fa"], "--devices expects"),
    (["a.fa", "b.fa"], "expected between 0 and 1 positional arguments but got 2"),
    (["does_not_exist.fa"], "Could not open file does_not_exist.fa"),
    (["-T", "does_not_exist.nwk", "{fasta}"], "Could not open file does_not_exist.nwk"),
    (["-C", "does_not_exist.yaml"], "Could not open file does_not_exist.yaml"),
    (["{one}"], "contains 1 sequence(s), cannot form an alignment"),
    (["{empty}"], "error: "),
])
def test_command_line_errors(tmp_path, args, message):
    files = {"fasta": ">a\nACGT\n>b\nACGA\n", "one": ">a\nACGTACGT\n", "empty": ""}
    for k, v in files.items():
        (tmp_path / (k + ".fa")).write_text(v)
    args = [a.format(**{k: str(tmp_path / (k + ".fa")) for k in files}) for a in args]
    r = run(args, cwd=str(tmp_path))
    assert r.returncode == 1 and r.stdout == b""
    assert message in r.stderr.decode()
    assert [ln for ln in r.stderr.decode().split("\n") if ln.startswith("error: ")]


def test_fasta_from_standard_input_with_one_sequence(tmp_path):
    r = subprocess.run([BIN, "-"], input=b">only\nACGT\n", capture_output=True, timeout=60)
    assert r.returncode == 1 and "FASTA input from STDIN contains 1 sequence(s)" in r.stderr.decode()


def test_help_exits_zero():
    r = run(["-h"])
    assert r.returncode == 0 and b"--tree / -T FILE" in r.stderr and b"--devices LIST" in r.stderr
    assert run(["--help"]).returncode == 0


def test_config_file_overrides_options_with_a_warning(tmp_path):
    cfg = tmp_path / "c.yaml"
    cfg.write_text(capi.Config().generate().replace("max_count: 3000", "max_count: 0"))   # no FASTA named either
    r = run(["-m", "5", "-C", str(cfg)])
    err = r.stderr.decode()
    assert r.returncode == 1 and "warning: All other command-line arguments are being overridden by config file parameters." in err
    assert "Invalid value for parameter 'max_count', got 0" in err   # the file's value, not -m 5
    r = run(["-C", str(cfg)])
    assert r.returncode == 1 and "warning" not in r.stderr.decode()


def _fields(s, prefix=""):
    """every leaf field of a ctypes structure as {dotted name: value}"""
    out = {}
    for name, typ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out.update(_fields(v, prefix + name + "."))
        elif isinstance(v, C.Array):
            for i, x in enumerate(v):
                out["%s%s[%d]" % (prefix, name, i)] = x
        elif typ is C.c_char_p:
            out[prefix + name] = v
        elif isinstance(typ, type) and issubclass(typ, C._Pointer):
            out[prefix + name] = bool(v)
        else:
            out[prefix + name] = v
    return out


def test_msa_params_of_the_defaults_are_the_librarys_defaults():
    lib = capi.load_library()
    want = capi.MsaParams()
    lib.cl_msa_params_default(C.byref(want))
    cfg = capi.Config()
    got = cfg.msa_params()
    assert _fields(got) == _fields(want)


def test_msa_params_of_a_changed_config():
    lib = capi.load_library()
    base = capi.MsaParams()
    lib.cl_msa_params_default(C.byref(base))
    cfg = capi.Config()
    changes = {
        # IO
        "subproblems_prefix": "sp", "restart": True, "all_pairs_prefix": "pw", "subalignments_filepath": "sub.txt", "threads": 5,
        # MatchFinding
        "max_count": 77, "use_color_set_size": False,
        # Anchoring
        "max_num_match_pairs": 4321, "memory_restraint_size": 12, "split_matches_at_branchpoints": False, "anchor_split_limit": 6,
        "min_split_length": 129, "min_path_length_spread": 51, "max_split_match_set_size": 17, "chaining_algorithm": 1,
        "anchor_gap_open": (1.5, 51, 5001), "anchor_gap_extend": (2.25, 0.2, 0.001), "anchor_score_function": 1, "pair_count_power": 0.75,
        "length_intercept": 2000, "length_decay_power": 1.5, "global_anchoring": False, "do_fill_in_anchoring": False,
        # IdentifyingAlignability
        "constraint_method": 2, "minimum_segment_score": 14000, "minimum_segment_average": 0.2, "window_length": 9000,
        "generalized_length_mean": -0.25, "boundary_score_factor": 0.9,
        # Aligning
        "stitch_match": 21, "stitch_mismatch": 81, "stitch_gap_open": (61, 801, 2501), "stitch_gap_extend": (31, 6, 2),
        "max_trivial_size": 30001, "min_wfa_size": 40000001, "max_wfa_size": 75000001, "max_wfa_ratio": 1.5, "wfa_pruning_dist": 26,
        "deletion_alignment_ratio": 9, "deletion_alignment_short_max_size": 1501, "deletion_alignment_long_min_size": 2001,
        "indel_fuzz_score_proportion": 0.002, "min_indel_fuzz_length": 51,
        # InducingCycles
        "cyclize_tandem_duplications": True, "max_tandem_duplication_search_rounds": 4, "min_cyclizing_length": 5000,
        "tandem_dup_score_proportion": 0.3, "include_tandem_dup_gap_scores": False, "deviation_drift_factor": 151,
        "separation_drift_factor": 51, "trim_window_proportion": 0.2, "deduplication_slosh_proportion": 0.15,
        "max_realignment_cycle_size": 10001, "inconsistent_indel_window": 101, "min_inconsistency_disjoint_length": 9,
        "min_inconsistency_total_length": 51, "realignment_min_padding": 1001, "realignment_max_padding": 10001,
        # DeveloperTools
        "bonds_prefix": "bd", "preserve_subproblems": True, "skip_calibration": True,
    }
    for k, v in changes.items():
        cfg[k] = v
    got = cfg.msa_params()
    score = {"gap_open": [1.5, 51, 5001], "gap_extend": [2.25, 0.2, 0.001], "anchor_score_function": 1, "pair_count_power": 0.75,
             "length_intercept": 2000.0, "length_decay_power": 1.5, "global_anchoring": 0}
    want = {"subproblems_prefix": b"sp", "restart": 1, "induced_pairwise_prefix": b"pw", "subalignments_path": b"sub.txt", "n_workers": 5,
            "merge.match.max_count": 77, "merge.match.use_color_set_size": 0,
            "merge.align.anchor.max_num_match_pairs": 4321, "merge.align.split_matches_at_branchpoints": 0,
            "merge.align.split.anchor_split_limit": 6, "merge.align.split.min_split_length": 129,
            "merge.align.split.min_path_length_spread": 51, "merge.align.split.max_split_match_set_size": 17,
            "merge.align.anchor.chaining_algorithm_plus_one": 2, "merge.align.anchor.do_fill_in_anchoring": 0,
            "merge.align.partition.constraint_method": 2, "merge.align.partition.minimum_segment_score": 14000.0,
            "merge.align.partition.minimum_segment_average": 0.2, "merge.align.partition.window_length": 9000.0,
            "merge.align.partition.generalized_length_mean": -0.25, "merge.align.partition.boundary_score_factor": 0.9,
            "merge.align.stitch.alignment_params.match": 21, "merge.align.stitch.alignment_params.mismatch": 81,
            "merge.align.stitch.max_trivial_size": 30001, "merge.align.stitch.min_wfa_size": 40000001,
            "merge.align.stitch.max_wfa_size": 75000001, "merge.align.stitch.max_wfa_ratio": 1.5, "merge.align.stitch.wfa_pruning_dist": 26,
            "merge.align.stitch.deletion_alignment_ratio": 9, "merge.align.stitch.deletion_alignment_short_max_size": 1501,
            "merge.align.stitch.deletion_alignment_long_min_size": 2001, "merge.align.indel_fuzz_score_proportion": 0.002,
            "merge.align.min_indel_fuzz_length": 51,
            "cyclize": 1, "max_tandem_duplication_search_rounds": 4, "bonds.min_length": 5000.0, "bonds.min_opt_proportion": 0.3,
            "bonds.include_gap_scores": 0, "bonds.deviation_drift_factor": 151.0, "bonds.separation_drift_factor": 51.0,
            "bonds.trim_window_proportion": 0.2, "bonds.deduplication_slosh_proportion": 0.15,
            "polish.max_tight_cycle_size": 10001, "polish.max_bond_inconsistency_window": 101, "polish.min_inconsistency_disjoint_length": 9,
            "polish.min_inconsistency_total_length": 51, "polish.padding_target_min_length": 1001, "polish.padding_max_length_limit": 10001,
            "bonds_prefix": b"bd", "skip_calibration": 1}
    for i in range(3):
        want["merge.align.stitch.alignment_params.gap_open[%d]" % i] = [61, 801, 2501][i]
        want["merge.align.stitch.alignment_params.gap_extend[%d]" % i] = [31, 6, 2][i]
    # one ScoreFunction in the reference: the match filter, the chaining and the partition read the same values
    for where in ("merge.match.score.", "merge.align.anchor.chain.", "merge.align.partition.score_function."):
        for k, v in score.items():
            if isinstance(v, list):
                for i in range(3):
                    want["%s%s[%d]" % (where, k, i)] = v[i]
            else:
                want[where + k] = v
    g, b = _fields(got), _fields(base)
    changed = {k: v for k, v in g.items() if b[k] != v}
    assert changed == want
    # the parameters with no effect here change no field: memory_restraint_size, preserve_subproblems (use_color_set_size is carried, unread)
    c2 = capi.Config()
    c2["memory_restraint_size"] = 5
    c2["preserve_subproblems"] = True
    assert _fields(c2.msa_params()) == b
    # the sparse-affine default keeps the struct's own spelling of it (0); exhaustive chaining maps to 1
    c2["chaining_algorithm"] = 0
    assert c2.msa_params().merge.align.anchor.chaining_algorithm_plus_one == 1


def test_msa_params_refuse_values_out_of_bounds():
    c = capi.Config()
    c["stitch_gap_open"] = (60, 50, 2500)
    with pytest.raises(capi.ClError) as e:
        c.msa_params()
    assert "increasing order" in str(e.value)
    c["fasta_name"] = "x.fa"
    with pytest.raises(capi.ClError) as e:
        c.validate()
    assert "increasing order" in str(e.value)
    c = capi.Config()
    c["fasta_name"] = "x.fa"
    c.validate()
    c["min_wfa_size"] = 80000000
    with pytest.raises(capi.ClError) as e:
        c.validate()
    assert "Got greater minimum than maximum" in str(e.value)


def test_config_get_and_set_errors():
    c = capi.Config()
    with pytest.raises(capi.ClError) as e:
        c["nope"] = 1
    assert "No parameter with name nope" in str(e.value)
    with pytest.raises(capi.ClError):
        c["nope"]
    assert c["anchor_gap_extend"] == "2.5,0.1,0.0015" and c["memory_restraint_size"] == "1073741824"
