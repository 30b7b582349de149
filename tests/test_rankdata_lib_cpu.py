"""tests/rankdata_lib.py against the O(n^2) definition of the three arrays for every dtype and both orders (both zeros and two NaN
payloads among the floats), and against scipy.stats.rankdata where scipy is installed."""
import numpy as np
import pytest

import oracle_lib as ol
import rankdata_lib as rl

ALL_DTYPES = [ol.U8, ol.U16, ol.U32, ol.U64, ol.I8, ol.I16, ol.I32, ol.I64, ol.F32, ol.F64]


def _keys(dt, n, seed):
    """n bit patterns of dtype dt with many duplicates, the sign bit in play, and for floats +-0.0 and two NaN payloads"""
    size = ol.DTYPE_SIZE[dt]
    top = 1 << (8 * size - 1)
    a = ol.splitmix_fill(n, dt, seed, top | (0x7 << (8 * size - 6)) | 0x3)
    if dt in (ol.F32, ol.F64) and n >= 16:
        nan = 0x7FC00000 if dt == ol.F32 else 0x7FF8000000000000
        special = np.array([0, top, nan, nan | 1, 0, top, nan], dtype=a.dtype)
        a[3:3 + special.size] = special
    return a


def _definition(bits, dt, order):
    k = ol.kdf_keys(bits, dt, order).astype(np.uint64)
    n = k.size
    lt = k[None, :] < k[:, None]                 # [i, j]: key j below key i
    eq = k[None, :] == k[:, None]
    earlier = np.tri(n, n, -1, dtype=bool)       # [i, j]: j < i
    less = lt.sum(axis=1)
    equal = eq.sum(axis=1)
    place = less + (eq & earlier).sum(axis=1)
    return place.astype(np.uint64), less.astype(np.uint64), equal.astype(np.uint64)


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt", ALL_DTYPES)
def test_against_the_definition(dt, order):
    for n in (1, 2, 77, 300):
        a = _keys(dt, n, 8600 + dt)
        place, less, equal = rl.want_rankdata(a, dt, order)
        dplace, dless, dequal = _definition(a, dt, order)
        assert np.array_equal(place, dplace) and np.array_equal(less, dless) and np.array_equal(equal, dequal), (dt, order, n)
        assert np.all(less <= place) and np.all(place < less + equal)
        assert np.array_equal(np.sort(place), np.arange(n, dtype=np.uint64))


def test_bit_equal_keys_only_are_equal():
    a = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0x00000000], dtype=np.uint32)   # +0.0, -0.0, two NaNs, +0.0
    place, less, equal = rl.want_rankdata(a, ol.F32)
    assert list(equal) == [2, 1, 1, 1, 2]
    assert list(less) == [1, 0, 3, 4, 1] and list(place) == [1, 0, 3, 4, 2]


def test_empty():
    place, less, equal = rl.want_rankdata(np.zeros(0, dtype=np.uint32), ol.U32)
    assert place.size == less.size == equal.size == 0


@pytest.mark.parametrize("method", ["ordinal", "min", "max", "average"])
def test_against_scipy(method):
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(8611)
    x = rng.integers(-20, 20, 300).astype(np.float32) / 4       # NaN-free, many ties, no zero of either sign but +0.0
    place, less, equal = rl.want_rankdata(x.view(np.uint32), ol.F32)
    got = rl.by_method(place, less, equal, method)
    want = stats.rankdata(x, method=method) - 1
    assert np.array_equal(np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64))
