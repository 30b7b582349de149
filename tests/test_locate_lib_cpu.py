"""tests/locate_lib.py against a brute-force double loop, without a GPU: the expected less / equal / bins of every GPU test of
rsx_sort_locate* come from locate_lib.Want, so Want itself is checked here against the definition -- counts of derived keys
compared one pair at a time -- on arrays of at most 200 keys: all ten dtypes, both orders, and f32 / f64 with NaNs of both signs,
+-0.0 and +-inf among keys and values.  Also from_kdf (the inverse of the oracle's kdf_keys) and search_shape on cases worked
out by hand."""
import numpy as np
import pytest

import locate_lib as ll
import oracle_lib as ol

SPECIAL = {ol.F32: [0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000],
           ol.F64: [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x0000000000000000, 0x8000000000000000,
                    0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000, 0xBFF0000000000000]}


def _data(dt, seed, n, m):
    rng = np.random.default_rng(seed)
    t = ol.NP_BITS[dt]
    top = 8 * ol.DTYPE_SIZE[dt]
    draw = lambda k: (rng.integers(0, 1 << 62, size=k, dtype=np.uint64) >> np.uint64(62 - min(top, 62))).astype(t) if top < 62 else \
        (rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)).astype(t)
    keys, vals = draw(n), draw(m)
    keys[: n // 3] &= t(0x3F)                                 # a crowd of small keys, so that values hit keys
    vals[: m // 2] = keys[rng.integers(0, n, size=m // 2)]    # half of the values occur among the keys
    if dt in SPECIAL:
        sp = np.array(SPECIAL[dt], dtype=t)
        keys[-sp.size:] = sp
        vals[-sp.size:] = sp[::-1]
    return keys, vals


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt", list(range(10)))
def test_want_against_the_definition(dt, order):
    for seed, n, m in ((1, 200, 60), (2, 37, 90), (3, 1, 12), (4, 64, 1)):
        if dt in SPECIAL and min(n, m) < len(SPECIAL[dt]):
            continue
        keys, vals = _data(dt, 100 * dt + seed, n, m)
        want = ll.Want(keys, dt, order)
        kk = [int(x) for x in ol.kdf_keys(keys, dt, order)]
        kv = [int(x) for x in ol.kdf_keys(vals, dt, order)]
        less, equal = want.at(vals)
        for j in range(m):
            assert less[j] == sum(1 for k in kk if k < kv[j]) and equal[j] == sum(1 for k in kk if k == kv[j]), (dt, order, j)
        at, below = want.bins(vals, False), want.bins(vals, True)
        for i in range(n):
            assert at[i] == sum(1 for v in kv if v <= kk[i]) and below[i] == sum(1 for v in kv if v < kk[i]), (dt, order, i)


def test_special_floats_are_distinct_keys():
    """-0.0 stands before +0.0, the NaNs at the two ends, by bit pattern"""
    for dt in (ol.F32, ol.F64):
        sp = np.array(SPECIAL[dt], dtype=ol.NP_BITS[dt])
        want = ll.Want(sp, dt, ol.ASC)
        less, equal = want.at(sp)
        assert list(equal) == [1] * sp.size and sorted(less) == list(range(sp.size))
        by = dict(zip([int(x) for x in sp], [int(x) for x in less]))
        assert by[SPECIAL[dt][4]] + 1 == by[SPECIAL[dt][3]]                 # -0.0 right before +0.0
        assert by[SPECIAL[dt][1]] == 0 and by[SPECIAL[dt][0]] == sp.size - 1   # -NaN first, +NaN last


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt", list(range(10)))
def test_from_kdf_inverts_the_oracle(dt, order):
    keys, _ = _data(dt, 77 + dt, 200, 20)
    assert np.array_equal(ll.from_kdf(ol.kdf_keys(keys, dt, order), dt, order), keys)


def test_search_shape_by_hand():
    u = lambda *a: np.array(a, dtype=np.uint32)
    assert ll.search_shape(u(5), ol.U32) == (1, 0, 0)
    assert ll.search_shape(u(5, 5, 5), ol.U32) == (1, 0, 0)
    assert ll.search_shape(u(6, 7), ol.U32) == (2, 0, 1)                     # one edge in the table
    assert ll.search_shape(u(0, 0xFFFFFFFF), ol.U32) == (2, 24, 1)
    # 100 edges in digit 0 and the last one far away: 100 in one span, 7 halvings
    assert ll.search_shape(np.concatenate([np.arange(100, dtype=np.uint32) * 2 + 5, u(0xC0000000)]), ol.U32) == (101, 24, 7)
    assert ll.search_shape(np.concatenate([np.arange(4095, dtype=np.uint64) + 1000, np.array([1 << 63], dtype=np.uint64)]), ol.U64) == (4096, 56, 12)
    # spread over the digits: 256 edges, one per digit (the last edge is not in the table)
    assert ll.search_shape((np.arange(256, dtype=np.uint32) << 24), ol.U32) == (256, 24, 1)
