"""The stitch plans the library MAKES for a fixed list of batches, as a table that two builds of the library can be compared by, byte for byte: parity of the alignments
does not notice a pair that moved to another (also correct) kernel or a launch that split in two.  Per batch: plan.stats() without n_strip_fallbacks, and per launch in
order kernel, n_problems, dp_cells, dp_bytes, lds_bytes, max_sweep, longest.  Plans are created and destroyed; nothing is executed.
Batches: the resident plan of bench.py (every stitch subproblem of the merges of its 10 x 1 Mbp MSA in one batch — the MSA runs once to get them), the ten batches of
scripts/stress_set.py, and a fixed-seed draw of --fuzz batches from the generators of scripts/fuzz_gpu.py (default scoring; NumPW as drawn there).  The table is made
once with the default switches and once per entry of CONFIGS (the plan-creation switches the tests and scripts set), each in a child process of its own (most of the
switches are read once per process).  The library is the one capi loads (CL_LIBRARY names another build); --batches FILE keeps the pickled batches for the next run,
so that two builds are given the very same inputs.
usage: python scripts/plan_table.py --out TABLE.json [--batches FILE] [--fuzz 200] [--length 1000000] [--jobs 4]; prints the table's sha256"""
import argparse
import hashlib
import json
import os
import pickle
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [
    {},
    {"CL_STITCH_PERSISTENT": "0"}, {"CL_STITCH_NARROW": "0"}, {"CL_NO_LANE": "1"}, {"CL_LINEAR_SPAN": "0"}, {"CL_LANE_WIDE": "1"},
    {"CL_LANE_WIDE": "1", "CL_LANE_MIN_SWEEP": "0"}, {"CL_RANK_ORDER": "lifo"}, {"CL_RANK_ORDER": "level"}, {"CL_LINEAR_DUOS": "0"}, {"CL_LINEAR_DUOS": "1"},
    {"CL_LANE_MIN_SWEEP": "0"}, {"CL_LANE_MAX_ROWS": "1024"}, {"CL_LANE_WAVES": "3"}, {"CL_LANE_WAVES": "4"}, {"CL_STITCH_WORKSPACE_WORDS": "60000"},
    {"CL_FORCE_GENERAL": "1"}, {"CL_NO_SYS": "1"}, {"CL_NO_STRIP": "1"},
]


def make_batches(length, n_fuzz):
    """[(name, StitchBatch, force_num_pw or None)]"""
    import numpy as np
    import bench
    from centrolign_amd import capi, msa, synth
    from scripts import fuzz_gpu
    out = []
    ctx = capi.Context(0)
    _, seqs, tree = synth.c3_workload(length)
    res = msa.progressive_msa(ctx, seqs, tree, workers=4, keep_merges=True)
    out.append(("bench", capi.StitchBatch.concat([b for _, b in bench.stitch_batches(res["stats"]["kept"])]), None))
    del res
    ctx.close()
    for n, count in ((32, 36000), (128, 2400), (512, 150), (2048, 10), (6300, 1)):
        for kind, kw in (("linear", dict(extra_edge_p=0.0, n_alt=0)), ("bubbles", dict(extra_edge_p=0.02, skip_max=2))):
            out.append(("stress %d^2 x %d %s" % (n, count, kind), synth.sized_dag_batch([(n, n)] * count, seed=9, **kw), None))
    rng = np.random.default_rng(20260)
    for i in range(n_fuzz):
        kind, seed, b, force, _ = fuzz_gpu.stitch_case(rng)
        out.append(("fuzz %d %s seed %d" % (i, kind, seed), b, force))
    return out


def tables(batches):
    from centrolign_amd import capi
    ctx = capi.Context(0)
    rows = []
    for name, b, force in batches:
        plan = ctx.plan(b, force_num_pw=force)
        st = plan.stats()
        st.pop("n_strip_fallbacks")
        launches = [{k: li[k] for k in ("kernel", "n_problems", "dp_cells", "dp_bytes", "lds_bytes", "max_sweep", "longest")} for li in plan.launches()]
        plan.destroy()
        rows.append({"batch": name, "stats": st, "launches": launches})
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--batches", default=None, help="pickle of the batches: made if the file does not exist, used as it is otherwise")
    ap.add_argument("--fuzz", type=int, default=200)
    ap.add_argument("--length", type=int, default=1000000)
    ap.add_argument("--jobs", type=int, default=4, help="child processes side by side")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        with open(args.child, "rb") as f:
            batches = pickle.load(f)
        with open(args.out, "w") as f:
            json.dump(tables(batches), f)
        return
    keep = args.batches is not None
    path = args.batches or tempfile.mkstemp(suffix=".pickle")[1]
    if not keep or not os.path.exists(path):
        # (in a child too: this process never opens the GPU, the children do)
        code = "import sys, pickle; sys.path.insert(0, %r); from scripts import plan_table as p; pickle.dump(p.make_batches(%d, %d), open(%r, 'wb'), protocol=4)" % (ROOT, args.length, args.fuzz, path)
        subprocess.check_call([sys.executable, "-c", code])
    result, running = {}, []
    todo = list(enumerate(CONFIGS))

    def reap(block):
        for item in list(running):
            i, cfg, proc, tmp = item
            if block or proc.poll() is not None:
                if proc.wait() != 0:
                    raise SystemExit("plan_table: the child for %r failed (%d)" % (cfg, proc.returncode))
                with open(tmp) as f:
                    result[i] = json.load(f)
                os.unlink(tmp)
                running.remove(item)
                block = False
    while todo or running:
        while todo and len(running) < max(1, args.jobs):
            i, cfg = todo.pop(0)
            tmp = tempfile.mkstemp(suffix=".json")[1]
            env = dict(os.environ, **cfg)
            running.append((i, cfg, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", path, "--out", tmp], env=env), tmp))
        reap(block=True)
    if not keep:
        os.unlink(path)
    text = json.dumps([{"switches": cfg, "plans": result[i]} for i, cfg in enumerate(CONFIGS)], indent=0, sort_keys=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("%s  %s  (%d configurations x %d batches)" % (hashlib.sha256(text.encode()).hexdigest(), args.out, len(CONFIGS), len(result[0])))


if __name__ == "__main__":
    main()
