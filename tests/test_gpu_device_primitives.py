"""GPU suite: the device primitives on their own — csrc/cl_radix.h's stable LSD radix sort (32- and 64-bit keys, any bit range) and inclusive prefix sum, and the
traceback's value index (csrc/chain_sort.hip) — element by element against NumPy.  Every comparison is exact; there is no tolerance anywhere.

The sizes are the smallest at which each branch of the kernels can go wrong (a tile is 2 048 keys, a wave's share 512, a round 64 lanes):
    0, 1, 2                 degenerate
    63, 64, 65              one round of a wave
    511, 512, 513           one wave's share of a tile
    2047, 2048, 2049        one tile / two
    4097                    three tiles, the last nearly empty
    524 288, 524 289        256 / 257 tiles: radix_rowscan_kernel with one / two table entries per thread
    2 097 152, 2 097 153    1 024 / 1 025 tiles: scan_sums_kernel with one / two tile sums per thread
    2 099 201               1 026 tiles: the last thread group of the scans partly filled
"""
import numpy as np
import pytest

from centrolign_amd import capi
from oracle import pyoracle as po
from tests.test_device_primitives import VALUE_INDEX_SIZES, check_value_index, value_sets

pytestmark = pytest.mark.gpu

SMALL_SIZES = (0, 1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097)
LARGE_SIZES = (524288, 524289, 2097152, 2097153, 2099201)
# pass counts 1 to 4 (8), so both parities of the ping-pong; last digits of width 1, 7, 8 and odd widths; begin_bit > 0
BIT_RANGES = {32: ((0, 32), (0, 1), (0, 7), (0, 9), (0, 17), (0, 31), (3, 20), (8, 16), (24, 32), (31, 32)),
              64: ((0, 64), (0, 8), (0, 33), (0, 42), (5, 64), (40, 64), (56, 64), (63, 64))}
DTYPE = {32: np.uint32, 64: np.uint64}
INVALID_ARGUMENT = -1   # CL_ERR_INVALID_ARGUMENT of include/centrolign_amd.h


def passes_of(begin, end):
    """(shift, width) of every 8-bit digit pass of a sort over bits [begin, end)"""
    return [(s, min(8, end - s)) for s in range(begin, end, 8)]


def _place(n, bits, begin, end, digit):
    """keys whose digit in pass p is digit(p, width) (an array of n values, cut to the pass's width); zero outside [begin, end)"""
    key = np.zeros(n, np.uint64)
    for p, (shift, width) in enumerate(passes_of(begin, end)):
        key |= (np.asarray(digit(p, width), np.uint64) & np.uint64((1 << width) - 1)) << np.uint64(shift)
    return key.astype(DTYPE[bits])


def _random_bits(n, bits, rng):
    return rng.integers(0, 1 << bits, n, dtype=np.uint64).astype(DTYPE[bits])


def _inside_mask(bits, begin, end):
    return DTYPE[bits](((1 << (end - begin)) - 1) << begin)


def d_uniform(n, bits, begin, end, rng):
    return _random_bits(n, bits, rng)


def d_all_equal(n, bits, begin, end, rng):
    """every pair in one bucket: the per-wave counters run to 512"""
    return np.full(n, _random_bits(1, bits, rng)[0], DTYPE[bits])


def d_two_digits(n, bits, begin, end, rng):
    def digit(p, width):
        pair = rng.integers(0, 1 << width, 2) if width > 1 else np.array([0, 1])
        return pair[rng.integers(0, 2, n)]
    return _place(n, bits, begin, end, digit)


def d_round_uniform(n, bits, begin, end, rng):
    """every round of 64 lanes holds one digit only: the peer mask is full, the lane == 63 edge of the ranking"""
    i = np.arange(n)
    return _place(n, bits, begin, end, lambda p, width: (i // 64) % 256)


def d_lane_distinct(n, bits, begin, end, rng):
    """every lane of a round a different digit (in the first pass; later passes see them gathered)"""
    i = np.arange(n)
    return _place(n, bits, begin, end, lambda p, width: i % 256)


def d_sorted(n, bits, begin, end, rng):
    return np.sort(_random_bits(n, bits, rng) & _inside_mask(bits, begin, end))


def d_reverse_sorted(n, bits, begin, end, rng):
    return d_sorted(n, bits, begin, end, rng)[::-1].copy()


def d_digits_00_ff(n, bits, begin, end, rng):
    return _place(n, bits, begin, end, lambda p, width: rng.integers(0, 2, n) * 0xFF)


def d_few_inside_random_outside(n, bits, begin, end, rng):
    """a handful of distinct values in the sorted bits, random bits outside them: stability and the carrying along of the untouched bits at once"""
    inside = _inside_mask(bits, begin, end)
    few = _random_bits(5, bits, rng) & inside
    return (_random_bits(n, bits, rng) & ~inside) | few[rng.integers(0, 5, n)]


DISTS = {f.__name__[2:]: f for f in (d_uniform, d_all_equal, d_two_digits, d_round_uniform, d_lane_distinct, d_sorted, d_reverse_sorted, d_digits_00_ff,
                                     d_few_inside_random_outside)}


def scrambled_values(n):
    """values that are no function of the position a pair ends up at: a sort that recomputed them instead of moving them would show"""
    return ((np.arange(n, dtype=np.uint64)[::-1] * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.uint32)


def reference_sort(keys, vals, begin, end):
    d = (keys.astype(np.uint64) >> np.uint64(begin)) & np.uint64((1 << (end - begin)) - 1)
    if end - begin <= 16:
        d = d.astype(np.uint16)   # (the same numbers; NumPy's stable sort of 16-bit integers is a radix sort, several times faster at 2 M keys)
    order = np.argsort(d, kind="stable")
    return keys[order], vals[order]


def check_sort(ctx, keys, vals, begin, end, what):
    want_k, want_v = reference_sort(keys, vals, begin, end)
    got_k, got_v = ctx.sort_pairs(keys, vals, begin, end)
    assert got_k.dtype == keys.dtype and got_v.dtype == np.uint32
    assert np.array_equal(got_v, want_v), "%s: the values are not the input's in stable order of key bits [%d, %d)" % (what, begin, end)
    assert np.array_equal(got_k, want_k), "%s: the keys did not travel whole with their values" % what


@pytest.mark.parametrize("dist", list(DISTS))
@pytest.mark.parametrize("bits", [32, 64])
def test_sort_small_sizes_every_bit_range(gpu_ctx, bits, dist):
    rng = np.random.default_rng([bits, list(DISTS).index(dist)])
    for n in SMALL_SIZES:
        vals = np.arange(n, dtype=np.uint32)
        for begin, end in BIT_RANGES[bits]:
            check_sort(gpu_ctx, DISTS[dist](n, bits, begin, end, rng), vals, begin, end, "%s, %d-bit, n = %d" % (dist, bits, n))


@pytest.mark.parametrize("bits", [32, 64])
def test_sort_all_distinct_digits_in_one_pass(gpu_ctx, bits):
    """one pass whose every round of 64 lanes holds 64 different digits: no lane has a peer, so the ranking inside a round decides nothing — the counters across
    rounds, waves and tiles alone place the keys"""
    for n in SMALL_SIZES + LARGE_SIZES[:2]:
        i = np.arange(n, dtype=np.uint64)
        for begin, end in [r for r in BIT_RANGES[bits] if 7 <= r[1] - r[0] <= 8]:
            keys = ((i % np.uint64(1 << (end - begin))) << np.uint64(begin)).astype(DTYPE[bits])
            check_sort(gpu_ctx, keys, scrambled_values(n), begin, end, "distinct digits, %d-bit, n = %d" % (bits, n))


@pytest.mark.parametrize("bits", [32, 64])
def test_sort_values_travel_with_their_keys(gpu_ctx, bits):
    for n in (513, 4097):
        rng = np.random.default_rng(n)
        for begin, end in BIT_RANGES[bits]:
            for dist in ("uniform", "few_inside_random_outside"):
                check_sort(gpu_ctx, DISTS[dist](n, bits, begin, end, rng), scrambled_values(n), begin, end, "%s, scrambled values, %d-bit, n = %d" % (dist, bits, n))


# what the large sizes are on the list for: the row scan of the digit table with two entries per thread (n > 524 288) under every kind of row — spread evenly,
# one full row, rows of two digits — and the sorts' share of the suffix rounds, the far pass and the value index at such sizes: each a few combinations
LARGE_CASES = (
    (64, "uniform", (0, 64), False),                      # eight passes: the suffix array's first round
    (64, "few_inside_random_outside", (5, 64), True),     # stability over 257 / 1 025 tiles, 64-bit, begin_bit > 0, an odd last digit (3 bits)
    (64, "all_equal", (40, 64), False),                   # one row of the table holds everything
    (32, "uniform", (0, 32), True),                       # the value index's sort
    (32, "few_inside_random_outside", (3, 20), False),    # stability, begin_bit > 0, a last digit of one bit
    (32, "round_uniform", (0, 9), False),                 # full peer masks in every round of every tile
    (32, "two_digits", (0, 17), False),
    (32, "digits_00_ff", (0, 31), False),                 # a 7-bit last digit after three whole ones
)


@pytest.mark.parametrize("n", LARGE_SIZES)
def test_sort_large_sizes(gpu_ctx, n):
    rng = np.random.default_rng(n)
    plain, scrambled = np.arange(n, dtype=np.uint32), scrambled_values(n)
    for bits, dist, (begin, end), scramble in LARGE_CASES:
        check_sort(gpu_ctx, DISTS[dist](n, bits, begin, end, rng), scrambled if scramble else plain, begin, end, "%s, %d-bit, n = %d" % (dist, bits, n))


def test_sort_fuzz(gpu_ctx):
    seed = 20261
    rng = np.random.default_rng(seed)
    names = list(DISTS)
    for case in range(200):
        bits = int(rng.choice([32, 64]))
        begin = int(rng.integers(0, bits))
        end = int(rng.integers(begin + 1, bits + 1))
        n = int(rng.integers(0, 10001))
        dist = names[int(rng.integers(0, len(names)))]
        vals = scrambled_values(n) if rng.integers(0, 2) else np.arange(n, dtype=np.uint32)
        check_sort(gpu_ctx, DISTS[dist](n, bits, begin, end, rng), vals, begin, end, "seed %d, case %d: %s, %d-bit, n = %d" % (seed, case, dist, bits, n))


def scan_inputs(n, rng):
    tiles = (n + 2047) // 2048
    first, last, tail = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    if n:
        first[0] = 1                                # every later tile adds the same 1
        last[-1] = 1
        tail[(tiles - 1) * 2048:] = 3               # zeros in every tile but the last: scan_add_kernel's early return in every workgroup
    return {
        "ones": np.ones(n, np.uint32),
        "flags_none": np.zeros(n, np.uint32),
        "flags_1e-6": (rng.random(n) < 1e-6).astype(np.uint32),
        "flags_half": (rng.random(n) < 0.5).astype(np.uint32),
        "first_only": first,
        "last_only": last,
        "last_tile_only": tail,
        "up_to_2^11": rng.integers(0, 1 << 11, n, dtype=np.uint32),   # the sum stays below 2^32 at these sizes
        "wrapping": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),   # wraps modulo 2^32 on purpose; the reference wraps too
    }


def check_scan(ctx, n):
    for name, values in scan_inputs(n, np.random.default_rng(n)).items():
        want = np.cumsum(values, dtype=np.uint64).astype(np.uint32)
        got = ctx.inclusive_sum(values)
        assert got.dtype == np.uint32 and np.array_equal(got, want), "inclusive sum of %s, n = %d, first differs at %s" % (name, n, np.flatnonzero(got != want)[:1])


def test_inclusive_sum_small_sizes(gpu_ctx):
    for n in SMALL_SIZES:
        check_scan(gpu_ctx, n)


@pytest.mark.parametrize("n", LARGE_SIZES)
def test_inclusive_sum_large_sizes(gpu_ctx, n):
    check_scan(gpu_ctx, n)


@pytest.mark.parametrize("n", VALUE_INDEX_SIZES)
def test_value_index_device_against_host_and_numpy(gpu_ctx, n):
    """the value index as a large DP builds it on the device, as a small DP builds it on the host, and NumPy's: all three the same arrays.  The values: normal
    x 1e3, small integers, +0.0 and -0.0 interleaved, CL_CHAIN_NEG, the smallest subnormals of both signs, +-FLT_MAX, each many times over.  NaN is left out:
    the DP never stores one."""
    for name, values in value_sets(n).items():
        keys, recs = gpu_ctx.chain_value_index(values)
        what = "%s, n = %d" % (name, n)
        check_value_index(values, keys, recs, "device index, " + what)
        host_keys, host_recs = capi.chain_value_index_host(values)
        assert np.array_equal(recs, host_recs) and np.array_equal(keys, host_keys), "device and host index differ: " + what


def test_suffix_array_past_the_scan_boundary(gpu_ctx):
    """a text of 2 097 153 + 5 000 characters: the doubling rounds run inclusive_sum over more than 1 024 tiles, as the root merges of a many-sequence MSA do.
    The oracle (po.oracle_suffix_array_lcp) takes 1.6 s of CPU time at this length (measured once, on the build machine; the longest common prefix is 22), well
    under the 10 s at which it would have to be left out: sa and lcp are compared with it outright, and verified from the text alone as well (0.6 s of NumPy): sa is a permutation, isa its inverse, the first lcp[p] characters at sa[p-1] and sa[p] agree and the next one
    strictly increases."""
    n = 2097153 + 5000
    rng = np.random.default_rng(7)
    text = rng.integers(1, 5, n).astype(np.uint8)
    text[-1] = 0
    sa, lcp, isa, rounds = gpu_ctx.suffix_array_lcp(text)
    assert rounds >= 2
    assert np.array_equal(np.sort(sa), np.arange(n, dtype=np.uint32)), "sa is not a permutation"
    assert np.array_equal(isa[sa], np.arange(n)), "isa is not the inverse of sa"
    assert lcp[0] == 0
    a, b, l = sa[:-1].astype(np.int64), sa[1:].astype(np.int64), lcp[1:].astype(np.int64)
    assert int(l.max()) < 64, "a random 4-letter text of this length has no repeat that long"
    for k in range(int(l.max())):
        m = l > k
        assert np.array_equal(text[a[m] + k], text[b[m] + k]), "character %d of a common prefix differs" % k   # (a + k < n: the unique last character ends every common prefix)
    pad = np.concatenate([text, np.zeros(1, np.uint8)])
    assert np.all(pad[np.minimum(a + l, n)] < pad[np.minimum(b + l, n)]), "suffixes out of order, or a common prefix longer than lcp says"
    want_sa, want_lcp = po.oracle_suffix_array_lcp(text)
    assert np.array_equal(sa, want_sa) and np.array_equal(lcp, want_lcp)


def _raises_invalid(ctx, rc):
    with pytest.raises(capi.ClError) as e:
        ctx._check(rc)
    assert e.value.code == INVALID_ARGUMENT and capi.ERRORS[e.value.code] == "CL_ERR_INVALID_ARGUMENT"
    return str(e.value)


def test_argument_errors_leave_the_context_usable(gpu_ctx):
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    k32, k64, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint64), np.arange(8, dtype=np.uint32)
    ko32, ko64, vo = np.full(8, 77, np.uint32), np.full(8, 77, np.uint64), np.full(8, 77, np.uint32)

    def sort(key_bytes, keys, vals, n, begin, end, keys_out, vals_out):
        ptr = lambda x: None if x is None else x.ctypes.data   # noqa: E731
        return lib.cl_device_sort_pairs(h, key_bytes, ptr(keys), ptr(vals), n, begin, end, ptr(keys_out), ptr(vals_out))
    for key_bytes in (0, 2, 3, 5, 16, -4):
        assert "key_bytes" in _raises_invalid(gpu_ctx, sort(key_bytes, k64, v, 8, 0, 8, ko64, vo))
    for begin, end in ((0, 0), (8, 8), (9, 3), (32, 32)):
        assert "end_bit" in _raises_invalid(gpu_ctx, sort(4, k32, v, 8, begin, end, ko32, vo))
    assert "end_bit" in _raises_invalid(gpu_ctx, sort(4, k32, v, 8, 0, 33, ko32, vo))
    assert "end_bit" in _raises_invalid(gpu_ctx, sort(8, k64, v, 8, 0, 65, ko64, vo))
    assert "2^32" in _raises_invalid(gpu_ctx, sort(4, k32, v, 1 << 32, 0, 32, ko32, vo))       # (refused before anything is read)
    assert "2^32" in _raises_invalid(gpu_ctx, sort(8, k64, v, (1 << 40) + 3, 0, 64, ko64, vo))
    for args in ((None, v, ko32, vo), (k32, None, ko32, vo), (k32, v, None, vo), (k32, v, ko32, None)):
        assert "null" in _raises_invalid(gpu_ctx, sort(4, args[0], args[1], 8, 0, 32, args[2], args[3]))
    assert "2^32" in _raises_invalid(gpu_ctx, lib.cl_device_inclusive_sum(h, v.ctypes.data, 1 << 32, vo.ctypes.data))
    assert "null" in _raises_invalid(gpu_ctx, lib.cl_device_inclusive_sum(h, None, 8, vo.ctypes.data))
    assert "null" in _raises_invalid(gpu_ctx, lib.cl_device_inclusive_sum(h, v.ctypes.data, 8, None))
    f = np.ones(8, np.float32)
    ki = np.full(8, 77, np.int32)
    assert "null" in _raises_invalid(gpu_ctx, lib.cl_chain_value_index(h, None, 8, ki.ctypes.data, vo.ctypes.data))
    assert "null" in _raises_invalid(gpu_ctx, lib.cl_chain_value_index(h, f.ctypes.data, 8, None, vo.ctypes.data))
    assert "null" in _raises_invalid(gpu_ctx, lib.cl_chain_value_index(h, f.ctypes.data, 8, ki.ctypes.data, None))
    assert np.all(ko32 == 77) and np.all(ko64 == 77) and np.all(vo == 77) and np.all(ki == 77), "a refused call wrote to its outputs"
    # n == 0: fine, and nothing is touched — not even looked at
    assert sort(4, None, None, 0, 0, 32, None, None) == 0 and sort(8, None, None, 0, 0, 64, None, None) == 0
    assert lib.cl_device_inclusive_sum(h, None, 0, None) == 0 and lib.cl_chain_value_index(h, None, 0, None, None) == 0
    # the same context still sorts
    rng = np.random.default_rng(5)
    for bits, (begin, end) in ((32, (3, 20)), (64, (0, 64))):
        check_sort(gpu_ctx, d_few_inside_random_outside(5000, bits, begin, end, rng), scrambled_values(5000), begin, end, "after the refusals, %d-bit" % bits)
    check_scan(gpu_ctx, 5000)
