"""tests/join_lib.py against a double loop: the oracle of the join tests is itself checked, on arrays of at most 40 rows, for u8,
i32, f32 (both zeros, two NaN payloads) and u64 keys, both orders, inner and left."""
import numpy as np
import pytest

import join_lib as jl
import oracle_lib as ol

F32_SPECIALS = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0x3F800000, 0xBF800000, 0x7F800000, 0xFF800000], dtype=np.uint32)


def _keys(dt, size, rng):
    if dt == ol.U8:
        return rng.integers(0, 7, size=size, dtype=np.uint64).astype(np.uint8) * np.uint8(37)
    if dt == ol.I32:
        return rng.choice(np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE, 12345], dtype=np.uint32), size=size)
    if dt == ol.F32:
        return rng.choice(F32_SPECIALS, size=size)
    return rng.choice(np.array([0, 1, 1 << 40, (1 << 64) - 1, 1 << 63, (1 << 40) + 1], dtype=np.uint64), size=size)


def _loops(left, right, dt, order):
    """The definitions of include/rsx.h, one comparison at a time."""
    kl = [int(k) for k in ol.kdf_keys(left, dt, order)]
    kr = [int(k) for k in ol.kdf_keys(right, dt, order)]
    perm = sorted(range(len(kr)), key=lambda j: (kr[j], j))
    start = [sum(1 for k in kr if k < x) for x in kl]
    count = [sum(1 for k in kr if k == x) for x in kl]
    return start, count, perm


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
@pytest.mark.parametrize("dt", [ol.U8, ol.I32, ol.F32, ol.U64])
def test_oracle_against_loops(dt, order):
    rng = np.random.default_rng(1000 + 10 * dt + order)
    for n, m in ((0, 0), (0, 5), (5, 0), (1, 1), (7, 3), (3, 7), (40, 40), (40, 13), (13, 40)):
        left, right = _keys(dt, n, rng), _keys(dt, m, rng)
        want = jl.Want(left, right, dt, order)
        start, count, perm = _loops(want.left, want.right, dt, order)
        assert [int(x) for x in want.start] == start and [int(x) for x in want.count] == count
        assert [int(x) for x in want.perm] == perm
        for left_join in (False, True):
            pl, pr = [], []
            for i in range(n):
                js = [j for j in range(m) if ol.kdf_keys(want.right[j:j + 1], dt, order)[0] == ol.kdf_keys(want.left[i:i + 1], dt, order)[0]]
                if not js and left_join:
                    js = [-1]
                pl += [i] * len(js)
                pr += js
            li, ri = want.pairs(left_join)
            assert list(li) == pl and list(ri) == pr, (n, m, left_join)
            assert want.n_pairs(left_join) == len(pl)


def test_bit_patterns_not_values():
    # -0.0 and +0.0 are two keys; a NaN matches the NaN of the same bits only
    left = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001], dtype=np.uint32)
    right = np.array([0x80000000, 0x7FC00001, 0x7FC00001, 0x00000000], dtype=np.uint32)
    want = jl.Want(left, right, ol.F32)
    assert list(want.count) == [1, 1, 0, 2]
    li, ri = want.pairs(True)
    assert list(li) == [0, 1, 2, 3, 3] and list(ri) == [3, 0, -1, 1, 2]


def test_pairs_of_takes_ranges_as_they_are():
    li, ri = jl.pairs_of([5, 0, 1], [0, 2, 1], [9, 8, 7], left_join=True)
    assert list(li) == [0, 1, 1, 2] and list(ri) == [-1, 9, 8, 8]
    li, ri = jl.pairs_of([5, 0, 1], [0, 2, 1], [9, 8, 7])
    assert list(li) == [1, 1, 2] and list(ri) == [9, 8, 8]
