"""The inputs of the chaining DP's sweep over the number of match pairs (tests/helpers.py:pair_cases()): every case holds exactly the pairs it states, its
combinations and records are the ones its family promises, and the driver's decisions predicted from the input alone — macro-blocks, far pass, levels of the far
pass's node tree, one packed block or separate arrays, query tables — fall on both sides of every count at which cl_chain_device.cpp, chain_device.h and
cl_chain_prep.cpp change what they do.  The oracle's values are reproducible and, where the compiled reference is built, its chain is the reference's.
The device side is tests/test_gpu_pair_sweep.py, which reads the same decisions from the library's own log."""
import hashlib

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H

CASES = H.pair_cases()
# family C at very few pairs: a pair lies in ONE of the sixteen combinations, so n pairs cover at most n of them; all sixteen from 255 pairs on
C_COMBOS_SMALL = {0: 0, 1: 1, 2: 2}
# the compiled reference's sparse_affine_chain_dp on these inputs: a few seconds at the most up to here
REF_MAX_PAIRS = {"A": 5121, "B": 2049, "C": 5121}


def by_family(family):
    return {c.n: H.pair_prediction(c) for c in CASES if c.family == family}


def test_the_cases_stand_on_both_sides_of_every_count():
    for fam in "ABC":
        pred = by_family(fam)
        for n in H.PAIR_COUNTS_ALL:
            assert n in pred
        # blocks of 256 and macro-blocks of 1 024: one short, full, one pair in the last
        assert all(n in pred for n in (255, 256, 257))
        for edge in (1024, 2048, 4096, 5120):
            assert (pred[edge - 1].n_macro, pred[edge].n_macro, pred[edge + 1].n_macro) == (edge // 1024, edge // 1024, edge // 1024 + 1)
        # the far pass at the default lag of 2 and, by the same rule, at lag 1
        assert not pred[4096].far and pred[4097].far and pred[4097].n_macro == 5
        assert (pred[3072].n_macro, pred[3073].n_macro) == (3, 4)
        assert not pred[1].packed or pred[1].pack_bytes <= H.PAIR_PACK_BYTES
        # packed and separate arrays on both sides of the family's pack edge
        assert {p.packed for p in pred.values() if p.pairs} == {True, False}, fam
    for fam in ("A", "C"):       # CL_CHAIN_FAR_LAG = 1, 3, 8
        for lag in H.PAIR_FAR_LAGS:
            assert (lag + 2) * 1024 in by_family(fam) and (lag + 2) * 1024 + 1 in by_family(fam)
    for fam in "ABC":
        edge, pred = H.PAIR_PACK_EDGE[fam], by_family(fam)
        assert pred[edge].packed and pred[edge].pack_bytes <= H.PAIR_PACK_BYTES < pred[edge + 1].pack_bytes and not pred[edge + 1].packed
        assert all(p.packed == (n <= edge) for n, p in pred.items() if n)
        assert all(p.walk == ("1" if n <= edge or fam == "C" else "2") for n, p in pred.items() if n)
    # family A: records = pairs, so the tree's levels change at exact pair counts, and 32 769 records take two top-level nodes
    a = by_family("A")
    assert [a[n].levels for n in (4097, 5121, 32767, 32768, 32769)] == [3, 3, 3, 4, 4]
    assert (a[32767].padded, a[32768].padded, a[32769].padded) == (32768, 32768, 65536)
    # every class of tree is reached with the far pass on
    levels = {p.levels for fam in "ABC" for p in by_family(fam).values() if p.far}
    assert levels == {1, 2, 3, 4}, levels
    c = by_family("C")
    assert c[4097].levels == 1 and c[32768].levels == 2 and 64 <= c[4097].largest < 512 <= c[32768].largest < 4096
    assert all(p.walk == "1" for p in c.values() if p.pairs)
    # dense | factored query tables: 16 combinations x 6 250 | 6 251 pairs
    assert c[6250].combos == c[6251].combos == 16 and not c[6250].factored and c[6251].factored
    assert a[32769].combos == 1 and not a[32769].factored


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_a_case_is_what_its_family_promises(case):
    g1, g2, ms, scale = H.pair_input(case)
    pred = H.pair_prediction(case)
    assert ms.n_pairs() == case.n == pred.pairs
    combos = H.count_combinations(g1, g2, ms)
    assert combos == pred.combos
    assert pred.records == H.count_records(g1, g2, ms)
    if case.family == "A":
        assert combos == min(case.n, 1) and pred.records == pred.largest == case.n
    elif case.family == "B":
        # four combinations from a few pairs on; a pair leaves a record in about every one of them
        assert combos == 4 if case.n >= 255 else 1 <= combos <= 4 if case.n else combos == 0
        assert (3.5 * case.n if case.n >= 255 else case.n) <= pred.records <= 4 * case.n
    else:
        assert combos == C_COMBOS_SMALL.get(case.n, 16) and pred.records == case.n
    assert pred.n_macro == -(-case.n // 1024)
    assert pred.far == (case.n > 4096)
    assert pred.levels == (1 if pred.largest < 512 else 2 if pred.largest < 4096 else 3 if pred.largest < 32768 else 4)
    assert pred.factored == (combos * case.n > 100000)


def oracle_digest(case, algo):
    g1, g2, ms, scale = H.pair_input(case)
    chain, dp = po.oracle_chain(algo, g1, g2, ms, scale=scale, want_dp=True, global_anchoring=True)
    h = hashlib.sha256(dp[:case.n].view(np.uint32).tobytes())
    h.update(np.ascontiguousarray(chain, np.uint32).tobytes())
    return h.hexdigest(), len(chain)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_values_are_reproducible(case):
    for algo in ("affine", "sparse"):
        first, second = oracle_digest(case, algo), oracle_digest(case, algo)
        assert first == second, (case.name, algo)
        assert case.n or first[1] == 0      # (no pair: an empty chain)


@pytest.mark.ref
@pytest.mark.parametrize("case", [c for c in CASES if c.n <= REF_MAX_PAIRS[c.family]], ids=repr)
def test_reference_agrees_with_the_live_oracle(case):
    g1, g2, ms, scale = H.pair_input(case)
    for algo in ("affine", "sparse"):
        for glob in (True, False):
            chain = po.oracle_chain(algo, g1, g2, ms, scale=scale, global_anchoring=glob)
            ref, _ = po.ref_chain(algo, g1, g2, ms, scale=scale, global_anchoring=glob)
            assert np.array_equal(ref, chain), (case.name, algo, glob)
