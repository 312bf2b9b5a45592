"""CPU suite: the host route of the chaining traceback's value index (capi.chain_value_index_host: the function ChainTrace::value_index runs for a small
DP) against NumPy — the order-preserving key of every value, the stable order, the decoding.  tests/test_gpu_device_primitives.py holds the device route
(and the radix sort and prefix sum under it) against the same references and the same inputs."""
import numpy as np
import pytest

from centrolign_amd import capi

F32 = np.finfo(np.float32)
CL_CHAIN_NEG = F32.min                       # csrc/chain_device.h: the DP's "no predecessor"
# Values are made from bit patterns and turned into float64 by integer arithmetic (as_float64): a library built with -ffast-math (the compiled reference of
# oracle/_ref is one) switches the thread that loads it to flushing subnormals to zero, and a test after it in the same process would then see 1e-45 == 0.
_bits = lambda *words: np.array(words, np.uint32).view(np.float32)   # noqa: E731
SUBNORMAL, NEG_SUBNORMAL = _bits(0x00000001, 0x80000001)             # the smallest positive and negative subnormals
VALUE_INDEX_SIZES = (0, 1, 64, 2049, 524289)   # nothing, one, one round of a wave, just past a tile, just past 256 tiles


def value_sets(n, seed=0):
    """{name: float32[n]}: the kinds of value a DP can store, each with many repeats — ties are the point.  No NaN: the DP never stores one (its values
    are sums and maxima of finite scores and CL_CHAIN_NEG), and the encoding gives NaN no place in the order."""
    rng = np.random.default_rng([seed, n])
    normal = (rng.standard_normal(max(n // 16, 1)) * 1e3).astype(np.float32)          # each drawn ~16 times below
    small = np.arange(-50, 51).astype(np.float32)
    edge = np.concatenate([np.array([0.0, -0.0, CL_CHAIN_NEG, F32.max, -F32.max], np.float32), _bits(0x00000001, 0x80000001)])
    pick = lambda pool: pool[rng.integers(0, len(pool), n)]   # noqa: E731
    zeros = np.zeros(n, np.float32)
    zeros[1::2] = -0.0                                                                 # +0.0 and -0.0 interleaved
    sets = {
        "normal": pick(normal),
        "small_integers": pick(small),
        "zeros_of_both_signs": zeros,
        "edges": pick(edge),
        "negatives_and_zeros": pick(np.concatenate([np.array([-0.0, 0.0, -1.0, -2.5, CL_CHAIN_NEG, -F32.max], np.float32), _bits(0x80000001)])),
        # a third of everything a zero of either sign, between ties of every other kind
        "mixed": pick(np.concatenate([normal[:64], small, edge, np.tile(np.array([0.0, -0.0], np.float32), 40)])),
        "all_chain_neg": np.full(n, CL_CHAIN_NEG, np.float32),
    }
    assert all(v.dtype == np.float32 and len(v) == n and not np.isnan(v).any() for v in sets.values())
    return sets


def as_float64(values):
    """values.astype(np.float64), exactly and whatever the thread's denormal mode: sign, exponent and mantissa put together with ldexp (no NaN, no infinity)"""
    b = values.view(np.uint32).astype(np.int64)
    e, m = (b >> 23) & 0xFF, b & 0x7FFFFF
    mag = np.where(e == 0, np.ldexp(m.astype(np.float64), -149), np.ldexp((m | 0x800000).astype(np.float64), (e - 150).astype(np.int32)))
    return np.where(b >> 31, -mag, mag)


def reference_keys(values):
    """the order-preserving integer key of every value: the float's bits, -0.0 folded onto +0.0, the low 31 bits flipped where negative"""
    b = values.view(np.int32).copy()
    b[b == -2**31] = 0
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def check_value_index(values, keys, recs, what):
    """(keys, recs) is the value index of `values`: exact against the NumPy reference, and the order once more from the values as float64"""
    key = reference_keys(values)
    order = np.argsort(key, kind="stable")
    assert recs.dtype == np.uint32 and keys.dtype == np.int32, what
    assert np.array_equal(recs, order), "%s: record order differs from the stable sort of the keys" % what
    assert np.array_equal(keys, key[recs]), "%s: keys differ" % what
    # +0.0 and -0.0 compare equal as numbers and stay in input order, so the two orders agree
    assert np.array_equal(recs, np.argsort(as_float64(values), kind="stable")), "%s: record order differs from the stable sort of the values" % what
    # decoding: the key gives the value back, except that -0.0 comes back as +0.0; the decoded keys do not decrease
    back = np.where(keys >= 0, keys, keys ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)
    want = values[recs].view(np.uint32).copy()
    want[want == 0x80000000] = 0
    assert np.array_equal(back.view(np.uint32), want), "%s: decoded keys are not the values" % what
    assert np.all(np.diff(as_float64(back)) >= 0), "%s: decoded keys decrease" % what


@pytest.mark.parametrize("n", VALUE_INDEX_SIZES)
def test_host_value_index_against_numpy(n):
    for name, values in value_sets(n).items():
        keys, recs = capi.chain_value_index_host(values)
        check_value_index(values, keys, recs, "%s, n = %d" % (name, n))


def test_reference_keys_order_the_edge_values():
    """the reference of the tests themselves: its keys put the edge values in their numeric order, CL_CHAIN_NEG first and the two zeros together"""
    v = np.concatenate([np.array([CL_CHAIN_NEG, -1.0], np.float32), _bits(0x80000001, 0x80000000, 0, 1), np.array([1.0, F32.max], np.float32)])
    assert np.array_equal(as_float64(v), [float(F32.min), -1.0, -2.0 ** -149, 0.0, 0.0, 2.0 ** -149, 1.0, float(F32.max)]) and np.signbit(as_float64(v)[3])
    k = reference_keys(v)
    assert k[3] == k[4] == 0 and np.all(np.diff(np.delete(k, 3)) > 0)
    assert k[0] == reference_keys(np.array([-F32.max], np.float32))[0] == k.min()


def test_host_value_index_argument_errors():
    lib = capi.load_library()
    v, k, r = np.ones(3, np.float32), np.zeros(3, np.int32), np.zeros(3, np.uint32)
    bad = -1
    assert capi.ERRORS[bad] == "CL_ERR_INVALID_ARGUMENT"
    assert lib.cl_chain_value_index_host(None, 3, k.ctypes.data, r.ctypes.data) == bad
    assert b"null array" in lib.cl_last_error(None)
    assert lib.cl_chain_value_index_host(v.ctypes.data, 3, None, r.ctypes.data) == bad
    assert lib.cl_chain_value_index_host(v.ctypes.data, 3, k.ctypes.data, None) == bad
    assert np.array_equal(k, np.zeros(3, np.int32)) and np.array_equal(r, np.zeros(3, np.uint32)), "a refused call wrote to its outputs"
    assert lib.cl_chain_value_index_host(None, 0, None, None) == 0          # nothing to index: fine, nothing touched
    keys, recs = capi.chain_value_index_host(np.zeros(0, np.float32))
    assert len(keys) == 0 and len(recs) == 0
    assert lib.cl_chain_value_index_host(v.ctypes.data, 3, k.ctypes.data, r.ctypes.data) == 0
    assert np.array_equal(r, np.arange(3)) and np.array_equal(k, np.full(3, np.float32(1.0).view(np.int32)))
