"""Child process of tests/test_gpu_far_modes.py: the chaining DP's far-pass switches (CL_CHAIN_FAR_MODE, CL_CHAIN_NO_FAR_PRUNE,
CL_CHAIN_OLD_WALK) are read once per process, so every variant runs in a process of its own on the same saved input and prints a
digest of every DP value and of the chain.

An input may carry rows of ChainParams fields (save_input(..., params=[...])): the DP is then run once per row, a "PARAMS <row>" line on stderr in front
of each run's timing log and one RESULT line per row; without them it runs once with the default parameters, global anchoring.

usage: python tests/far_ab_child.py INPUT.npz affine|sparse"""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from centrolign_amd import capi  # noqa: E402

GRAPH_KEYS = ("label", "next_off", "next_idx", "prev_off", "prev_idx", "path_off", "path_nodes")


def params_row(p):
    return list(p.gap_open) + list(p.gap_extend) + [p.anchor_score_function, p.pair_count_power, p.length_intercept, p.length_decay_power, p.global_anchoring]


def params_from_row(row):
    p = capi.default_chain_params()
    p.gap_open[:] = [float(x) for x in row[0:3]]
    p.gap_extend[:] = [float(x) for x in row[3:6]]
    p.anchor_score_function = int(row[6])
    p.pair_count_power, p.length_intercept, p.length_decay_power = float(row[7]), float(row[8]), float(row[9])
    p.global_anchoring = int(row[10])
    return p


def save_input(path, g1, g2, ms, scale, params=None, extra=None):
    d = {"scale": np.array([scale])}
    d.update(extra or {})      # (further arrays a child of its own reads: tests/pair_sweep_child.py)
    if params is not None:
        d["params"] = np.array([params_row(p) for p in params], np.float64).reshape(-1, 11)
    for tag, g in (("g1.", g1), ("g2.", g2)):
        for k in GRAPH_KEYS:
            d[tag + k] = getattr(g, k)
        d[tag + "tableau"] = np.array([g.src_id, g.snk_id], np.uint64)
    for k in capi.MatchSets._DT:
        d["ms." + k] = getattr(ms, k)
    np.savez(path, **d)


def load_input(path):
    z = np.load(path)
    graphs = []
    for tag in ("g1.", "g2."):
        t = z[tag + "tableau"]
        graphs.append(capi.BaseGraph(*[z[tag + k] for k in GRAPH_KEYS], int(t[0]), int(t[1])))
    ms = capi.MatchSets(**{k: z["ms." + k] for k in capi.MatchSets._DT})
    return graphs[0], graphs[1], ms, float(z["scale"][0])


def load_params(path):
    z = np.load(path)
    return [params_from_row(r) for r in z["params"]] if "params" in z.files else None


def digests(dp, chain):
    return hashlib.sha256(dp.view(np.uint32).tobytes()).hexdigest(), hashlib.sha256(np.ascontiguousarray(chain).tobytes()).hexdigest()


def main():
    g1, g2, ms, scale = load_input(sys.argv[1])
    rows = load_params(sys.argv[1])
    sparse = sys.argv[2] == "sparse"
    ctx = capi.Context(0)
    for k, p in enumerate(rows if rows is not None else [capi.default_chain_params(global_anchoring=True)]):
        if rows is not None:
            print("PARAMS %d" % k, file=sys.stderr, flush=True)
        got = ctx.chain_sparse_affine(g1, g2, ms, scale=scale, want_dp=True, sparse=sparse, params=p)
        print("RESULT pairs=%d anchors=%d dp=%s chain=%s device_ms=%.1f" % ((got["n_pairs"], len(got["chain"])) + digests(got["dp"], got["chain"]) + (got["device_ms"],)), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
