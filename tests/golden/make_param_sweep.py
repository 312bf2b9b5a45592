#!/usr/bin/env python3
"""Regenerates tests/golden/popoa_param_sweep.npz and tests/golden/chain_param_sweep.npz from the COMPILED REFERENCE (oracle/_ref, `make -C
oracle ref`): the reference's results at every named scoring-parameter point of tests/helpers.py (STITCH_SET_NAMES, CHAIN_SETS).  Results
only; the inputs are rebuilt from seeds by helpers.sweep_stitch_batches() / helpers.sweep_chain_cases().

  popoa_param_sweep.npz   per set and batch: po_poa<1|2|3> on every pair (alignment lengths, a 64-bit digest of every alignment, scores) and
                          Stitcher::subalign (NumPW as chosen) wherever the reference's choice is defined
  chain_param_sweep.npz   per set, scale and anchoring: sparse_affine_chain_dp's chain; per set and anchoring: sparse_chain_dp's chain

Two things the reference leaves undefined are recorded as such instead of as results:
* Stitcher::subalign divides by (gap_extend[i-1] - gap_extend[i]) when it derives the piece cutoffs (src/stitcher.cpp:39-43): with two equal
  neighbouring extends that is an integer division by zero.  For those sets ("subalign_defined" == 0: edit, free_gaps, equal_pieces and the
  random draws with a repeated extend) only the forced-NumPW results exist; the library answers them with CL_ERR_BAD_GAP_PARAMS.
* the reference does not report the NumPW, the route or the score of Stitcher::subalign.  The stored num_pw, route and score of the "sub." leg are
  the oracle's (on those three fields the CPU test compares the oracle with itself; the alignments are the reference's); the generator checks that, for
  every device-routed pair, the reference's subalign alignment is the reference's po_poa<num_pw> alignment — which cannot tell two NumPW apart where
  they give the same alignment.  The forced legs' scores are the reference's.

The files are written with fixed zip timestamps, so a re-run reproduces them byte for byte."""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import pyoracle as po  # noqa: E402
from tests import helpers as H  # noqa: E402


def save_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), version=(1, 0))
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def stitch_goldens():
    out = {}
    batches = H.sweep_stitch_batches()
    out["set_names"] = np.array(H.STITCH_SET_NAMES)
    out["batch_names"] = np.array(sorted(batches))
    for name in H.STITCH_SET_NAMES:
        for bname, b in sorted(batches.items()):
            p = H.stitch_params(name, b)            # (asserts the domain condition)
            pre = "%s/%s/" % (name, bname)
            out[pre + "values"] = np.array(H.alignment_values(p), np.int64)
            forced = {}
            for npw in (1, 2, 3):
                f = np.full(b.n_problems, npw, np.uint8)
                ref, _ = po.ref_stitch_batch(b, p, force_num_pw=f)
                ref.route = po.oracle_stitch_batch(b, p, force_num_pw=f).route
                forced[npw] = ref
                out.update(H.pack_sweep_result(ref, pre + "pw%d." % npw))
            defined = H.subalign_defined(p)
            out[pre + "subalign_defined"] = np.array([int(defined)], np.uint8)
            if not defined:
                continue
            ref, _ = po.ref_stitch_batch(b, p)
            orc = po.oracle_stitch_batch(b, p)
            ref.route, ref.num_pw, ref.score = orc.route, orc.num_pw, orc.score
            for k in np.flatnonzero(orc.route == 0):
                assert np.array_equal(ref.alignment(k), forced[int(orc.num_pw[k])].alignment(k)), (name, bname, int(k))
            out.update(H.pack_sweep_result(ref, pre + "sub."))
        print("stitch", name)
    save_npz(os.path.join(HERE, "popoa_param_sweep.npz"), out)


def chain_goldens():
    out = {}
    cases = H.sweep_chain_cases()
    out["set_names"] = np.array(sorted(H.CHAIN_SETS))
    for name in sorted(H.CHAIN_SETS):
        for glob in (False, True):
            p = H.chain_params(name, glob)
            for cname, g1, g2, ms in cases:
                pre = "%s/%s/%s/" % (name, "global" if glob else "local", cname)
                out[pre + "sparse"], _ = po.ref_chain("sparse", g1, g2, ms, params=p, global_anchoring=glob)
                for scale in H.CHAIN_SCALES:
                    out[pre + "affine@%g" % scale], _ = po.ref_chain("affine", g1, g2, ms, scale=scale, params=p, global_anchoring=glob)
        print("chain", name)
    save_npz(os.path.join(HERE, "chain_param_sweep.npz"), out)


if __name__ == "__main__":
    stitch_goldens()
    chain_goldens()
