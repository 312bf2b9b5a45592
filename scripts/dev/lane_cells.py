"""which cell the steps of popoa_lane_kernel take, and what the general ones needed: a host-side model that replays the kernel's own rule (popoa_lane.h: the
ballot over `slow` per wave and step) from the row and column records of choose_lane (cl_stitch_plan_api.cpp), strip by strip and step by step, for every near-chain
pair of the bench step's plan (bench_data/c3_batches.npz, scripts/dev/dump_c3_batches.py) that sweeps CL_LANE_MIN_SWEEP rows + columns and more.

Per pair: wave-steps on the usual and on the general cell; the general ones by the class a tiered cell would give them (row-general over chain columns, column-general
over chain rows, both, a saved-column predecessor) and by what their active lanes needed (row distances > 1, column distances 2-3, a source row / column, a saved
column read / written); how many of the general wave-steps lie in CHUNKS whose columns are all plain (the per-chunk rule of the tiered cell); the macro-steps of
lane_body with its extra rounds; and a predicted duration from instructions per step (usual ~100, general ~230, 4 cycles each at 2.4 GHz, a macro-step as long as
its slowest wave).  With --alone N the N longest are also run alone on the device (as lane_probe.py does) and their own-clock time printed beside the prediction.
usage: python scripts/dev/lane_cells.py [--npz PATH] [--alone N [--label TEXT] [--tree DIR] [--append]] [--out FILE] [--synthetic]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# --tree DIR: the checkout whose built library is loaded (the model is this script's; with --alone the pairs then run on that tree's kernels — a parent commit's, say)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from centrolign_amd import capi, synth  # noqa: E402

CHUNK, LAG, USUAL_INSTR, GENERAL_INSTR, GHZ = 32, 3, 100, 230, 2.4


def side_records(batch, k, side):
    """the side's nodes in the device's rank order: (predecessor ranks + 1 per node, source flags, labels), or None for an empty side"""
    s = batch.side[side]
    b, e = int(s.node_off[k]), int(s.node_off[k + 1])
    n = e - b
    if n == 0:
        return None
    order = capi.stitch_rank_order(batch, k, side)[0]
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    preds = []
    for r in range(n):
        v = b + int(order[r])
        preds.append(sorted(int(rank[p]) + 1 for p in s.prev_idx[int(s.prev_off[v]):int(s.prev_off[v + 1])]))
    src = np.zeros(n, bool)
    src[rank[s.src_idx[int(s.src_off[k]):int(s.src_off[k + 1])].astype(np.int64)]] = True
    return preds, src, s.label[b:e][order]


def lane_records(batch, k, min_sweep=512, max_rows=1024):
    """choose_lane's rowrec / colrec of pair k (without the LDS ceiling), or None where the register kernel does not take the pair"""
    n = [int(batch.side[s].node_off[k + 1] - batch.side[s].node_off[k]) for s in (0, 1)]
    if min(n) == 0 or min(n) > max_rows or n[0] + n[1] < min_sweep:
        return None
    s_row = 1 if n[1] < n[0] else 0
    rows, cols = side_records(batch, k, s_row), side_records(batch, k, 1 - s_row)

    def chain(sd):
        preds, src, _ = sd
        return src[0] and src.sum() == 1 and not preds[0] and all(p == [i] for i, p in enumerate(preds[1:], 1))
    if chain(rows) and chain(cols):
        return None   # a chain pair: the chain kernels'
    rp, rsrc, rlab = rows
    cp, csrc, clab = cols
    n_r, n_c = len(rp), len(cp)
    max_rd = max([i + 1 - q for i, p in enumerate(rp) for q in p] + [0])
    if max_rd > 4 or any(not p and not rsrc[i] for i, p in enumerate(rp)):
        return None
    far = sorted({q for j, p in enumerate(cp) for q in p if j + 1 - q > 3})
    if len(far) > 16 or any(sum(j + 1 - q > 3 for q in p) > 2 for j, p in enumerate(cp)) or any(not p and not csrc[j] for j, p in enumerate(cp)):
        return None
    rowrec = np.zeros(n_r, np.uint32)
    for i, p in enumerate(rp):
        rowrec[i] = sum(1 << (i - q) for q in p) | (int(rsrc[i]) << 4) | ((int(rlab[i]) & 0x7F) << 8)
    colrec = np.zeros(n_c, np.uint32)
    for j, p in enumerate(cp):
        near = sum(1 << (j - q) for q in p if j + 1 - q <= 3)
        nf = sum(j + 1 - q > 3 for q in p)
        colrec[j] = near | (int(csrc[j]) << 4) | (nf << 5) | ((int(clab[j]) & 0x7F) << 8) | ((1 << 15) if (j + 1) in far else 0)
    return dict(k=k, nR=n_r, nC=n_c, DR=2 if max_rd <= 2 else 4, rowrec=rowrec, colrec=colrec, saved=len(far))


def replay(rec, waves):
    """the kernel's rule per strip and step; returns the counts of one pair in a workgroup of `waves` waves (1 for pairs of at most 64 rows)"""
    n_r, n_c = rec["nR"], rec["nC"]
    w = 1 if n_r <= 64 else waves
    rowrec = rec["rowrec"].copy()
    rowrec[0] = (rowrec[0] & ~np.uint32(0x1F)) | 1      # the first row's only predecessor is the boundary row: a chain row for the cell
    colrec = rec["colrec"]
    s_n, c_n = (n_r + 63) // 64, (n_c + 63 + CHUNK - 1) // CHUNK
    t_n = c_n * CHUNK
    pm = max(c_n, LAG * w)
    macro = ((s_n - 1) // w) * pm + LAG * ((s_n - 1) % w) + c_n
    out = dict(rows=n_r, cols=n_c, waves=w, strips=s_n, macro=macro, steps=macro * CHUNK, wave_steps=s_n * t_n, usual=0, general=0, slow_strips=0,
               cls_row=0, cls_row_src=0, cls_col=0, cls_both=0, cls_far=0, need_rd=0, need_c23=0, need_rsrc=0, need_csrc=0, need_far=0, need_save=0,
               chunk_plain_general=0)
    nonplain_col = np.concatenate([[False], (colrec & 0x7F) != 1])     # by 1-based column
    chunk_cost = np.zeros((s_n, c_n))
    t = np.arange(t_n)[:, None]
    for s in range(s_n):
        rr = rowrec[s * 64:min(n_r, s * 64 + 64)]
        nl = len(rr)
        lane = np.arange(nl)[None, :]
        b = t - lane + 1
        active = (b >= 1) & (b <= n_c)
        cr = np.where(active, colrec[np.clip(b - 1, 0, n_c - 1)], 0).astype(np.uint32)
        rowslow = ((rr & 0x1F) != 1)[None, :]
        colslow = active & ((cr & 0x7F) != 1)
        slow_row_t = (active & rowslow).any(1)
        slow_col_t = colslow.any(1)
        general = slow_row_t | slow_col_t
        far_t = (active & (((cr >> 5) & 3) != 0)).any(1)
        rsrc_t = (active & (((rr >> 4) & 1) != 0)[None, :]).any(1)
        out["slow_strips"] += bool(rowslow.any())
        out["general"] += int(general.sum())
        out["usual"] += int(t_n - general.sum())
        out["cls_far"] += int((general & far_t).sum())
        out["cls_row"] += int((general & ~far_t & ~slow_col_t).sum())
        out["cls_row_src"] += int((general & ~far_t & ~slow_col_t & rsrc_t).sum())
        out["cls_col"] += int((general & ~far_t & slow_col_t & ~slow_row_t).sum())
        out["cls_both"] += int((general & ~far_t & slow_col_t & slow_row_t).sum())
        out["need_rd"] += int((general & (active & ((rr & 0xE) != 0)[None, :]).any(1)).sum())
        out["need_c23"] += int((general & (active & ((cr & 6) != 0)).any(1)).sum())
        out["need_rsrc"] += int((general & rsrc_t).sum())
        out["need_csrc"] += int((general & (active & (((cr >> 4) & 1) != 0)).any(1)).sum())
        out["need_far"] += int((general & far_t).sum())
        out["need_save"] += int((general & (active & (((cr >> 15) & 1) != 0)).any(1)).sum())
        # the tiered cell's chunk rule: the columns in the strip's lanes when the chunk begins and the 32 it fetches
        for c in range(c_n):
            t0 = c * CHUNK
            lo, hi = max(1, t0 - nl + 1), min(n_c, t0 + CHUNK)
            plain = hi < lo or not nonplain_col[lo:hi + 1].any()
            g = int(general[t0:t0 + CHUNK].sum())
            if plain:
                out["chunk_plain_general"] += g
            chunk_cost[s, c] = g * GENERAL_INSTR + (CHUNK - g) * USUAL_INSTR
    # a macro-step lasts as long as its slowest wave (the barrier per chunk)
    instr = 0.0
    for m in range(macro):
        worst = 0.0
        for wv in range(w):
            mm = m - LAG * wv
            if mm < 0:
                continue
            j, c = divmod(mm, pm)
            s = j * w + wv
            if s < s_n and c < c_n:
                worst = max(worst, chunk_cost[s, c])
        instr += worst
    out["pred_ms"] = instr * 4 / (GHZ * 1e6)
    return out


def alone_ms(ctx, batch, k, waves):
    os.environ["CL_LANE_MIN_SWEEP"] = "0"
    os.environ["CL_LANE_WAVES"] = str(waves)
    try:
        plan = ctx.plan(batch.subset(np.array([k])))
        for _ in range(3):
            plan.execute(); plan.sync()
        best, kern = 1e9, ""
        for _ in range(5):
            plan.execute(); plan.sync()
            for li in plan.launches():
                if li["n_problems"]:
                    best, kern = min(best, li["in_pass_ms"]), li["kernel"]
        plan.destroy()
        return best, kern
    finally:
        os.environ.pop("CL_LANE_MIN_SWEEP", None)
        os.environ.pop("CL_LANE_WAVES", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--npz", default=os.path.join(ROOT, "bench_data", "c3_batches.npz"))
    ap.add_argument("--alone", type=int, default=0, help="run the N longest alone on the device and print their own-clock time")
    ap.add_argument("--waves", type=int, default=3, help="waves of a round in the plan (plans of 2 048 subproblems and more: 3)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=None, help="load the library of this checkout instead (see above)")
    ap.add_argument("--label", default=None, help="names the build in the heading of the --alone block (default: the CL_LANE_CELLS setting)")
    ap.add_argument("--append", action="store_true", help="with --alone and --out: append only the --alone block to the file (the table is already there)")
    ap.add_argument("--synthetic", action="store_true", help="synth.near_chain_batch([(165, 2225), (35, 2130), (433, 441)], p_snp=0.01, p_del=0.005) instead of the bench step's batches (no device)")
    args = ap.parse_args()
    if args.synthetic:
        batch = synth.near_chain_batch([(165, 2225), (35, 2130), (433, 441)], p_snp=0.01, p_del=0.005)
    else:
        from step_launches import load_batch
        batch = load_batch(args.npz)
    n1, n2 = batch.sizes()
    cand = np.flatnonzero((n1 + n2 >= 512) & (np.minimum(n1, n2) >= 1) & (np.minimum(n1, n2) <= 1024))
    rows = []
    for k in cand:
        rec = lane_records(batch, int(k))
        if rec is not None:
            r = replay(rec, args.waves)
            r["k"], r["DR"], r["saved"] = int(k), rec["DR"], rec["saved"]
            rows.append(r)
    rows.sort(key=lambda r: -r["pred_ms"])
    lines = ["near-chain pairs of %d subproblems that the register kernel takes (rows + columns >= 512): %d, %d of them in one wave, %d in rounds of %d waves" %
             (batch.n_problems, len(rows), sum(r["waves"] == 1 for r in rows), sum(r["waves"] > 1 for r in rows), args.waves),
             "wave-steps: strips x steps of a strip.  usual / general: the cell the kernel's ballot gives the wave-step.  classes of the general ones: row = slow rows over plain chain columns",
             "(src: with a source row among the active lanes), col = chain rows at a column that is not a plain chain column, both, far = a saved-column predecessor.  needs: general wave-steps",
             "in which an active lane had a row distance > 1 (rd), a column distance 2-3 (c23), a source row / column (rsrc / csrc), a saved-column read (far) or write (save).",
             "chunk-plain: general wave-steps inside chunks whose columns (those in the strip's lanes and the 32 fetched) are all plain chain columns.  pred: sum over macro-steps of",
             "the slowest wave's instructions (usual %d, general %d per step) x 4 cycles at %.1f GHz.  steps = macro-steps x 32 (extra rounds of pairs above %d rows included)." % (USUAL_INSTR, GENERAL_INSTR, GHZ, 64 * args.waves),
             "",
             "%7s %5s %5s %2s %2s %3s %5s %6s | %7s %7s %7s %5s | %6s %6s %6s %6s %6s | %6s %6s %6s %6s %6s %6s | %7s | %7s" %
             ("problem", "rows", "cols", "DR", "W", "S", "macro", "steps", "wave-st", "usual", "general", "gen%", "row", "rowsrc", "col", "both", "far", "rd", "c23", "rsrc", "csrc", "far", "save", "chunk-p", "pred ms")]
    for r in rows:
        lines.append("%7d %5d %5d %2d %2d %3d %5d %6d | %7d %7d %7d %5.1f | %6d %6d %6d %6d %6d | %6d %6d %6d %6d %6d %6d | %7d | %7.3f" %
                     (r["k"], r["rows"], r["cols"], r["DR"], r["waves"], r["strips"], r["macro"], r["steps"], r["wave_steps"], r["usual"], r["general"], 100.0 * r["general"] / max(1, r["wave_steps"]),
                      r["cls_row"], r["cls_row_src"], r["cls_col"], r["cls_both"], r["cls_far"], r["need_rd"], r["need_c23"], r["need_rsrc"], r["need_csrc"], r["need_far"], r["need_save"],
                      r["chunk_plain_general"], r["pred_ms"]))
    tot = {f: sum(r[f] for r in rows) for f in ("wave_steps", "usual", "general", "cls_row", "cls_col", "cls_both", "cls_far", "chunk_plain_general")}
    lines += ["", "all pairs: %(wave_steps)d wave-steps, %(usual)d usual, %(general)d general (row %(cls_row)d, col %(cls_col)d, both %(cls_both)d, far %(cls_far)d; chunk-plain %(chunk_plain_general)d)" % tot]
    by_sweep = sorted(rows, key=lambda r: -(r["rows"] + r["cols"]))
    lines.append("order of the five longest by rows + columns: %s; by predicted time: %s" % ([r["k"] for r in by_sweep[:5]], [r["k"] for r in rows[:5]]))
    if args.alone:
        ctx = capi.Context(0)
        if args.append:
            lines = []
        lines += ["", "alone on the device, the kernel's own clock (best of 5 passes), %s:" % (args.label or "CL_LANE_CELLS=%s" % os.environ.get("CL_LANE_CELLS", "(default)"))]
        for r in rows[:args.alone]:
            ms, kern = alone_ms(ctx, batch, r["k"], args.waves)
            lines.append("%7d %5d x %5d  %-24s %.3f ms alone = %.3f us per step of %d   (predicted %.3f ms, general %.1f %%)" %
                         (r["k"], r["rows"], r["cols"], kern, ms, ms * 1e3 / r["steps"], r["steps"], r["pred_ms"], 100.0 * r["general"] / max(1, r["wave_steps"])))
        ctx.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
