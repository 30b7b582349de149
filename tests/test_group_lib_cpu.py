"""tests/group_lib.py against numpy: np.unique on unsigned keys (where numpy's order is the KDF's), and the identities that
define the four arrays on floats with both zeros and two NaN payloads."""
import numpy as np
import pytest

import group_lib as gr
import oracle_lib as ol


@pytest.mark.parametrize("dt,mask,n", [(ol.U32, 0x00F0FF0F, 5003), (ol.U8, 0xFF, 3001), (ol.U64, 0x3FFFF, 4099), (ol.U16, 0xFFFF, 70001)])
def test_against_np_unique(dt, mask, n):
    a = ol.splitmix_fill(n, dt, 8101, mask)
    inv, keys, counts, first = gr.want_group(a, dt)
    k, idx, ninv, cnt = np.unique(a, return_index=True, return_inverse=True, return_counts=True)
    assert np.array_equal(keys, k) and np.array_equal(inv, ninv.reshape(-1)) and np.array_equal(counts, cnt)
    assert np.array_equal(first, idx)


def test_descending_reverses_the_groups():
    a = ol.splitmix_fill(4001, ol.U32, 8102, 0x3FF)
    inv, keys, counts, first = gr.want_group(a, ol.U32, ol.DESC)
    k, idx, ninv, cnt = np.unique(a, return_index=True, return_inverse=True, return_counts=True)
    g = k.size
    assert np.array_equal(keys, k[::-1]) and np.array_equal(inv, g - 1 - ninv.reshape(-1))
    assert np.array_equal(counts, cnt[::-1]) and np.array_equal(first, idx[::-1])


@pytest.mark.parametrize("order", [ol.ASC, ol.DESC])
def test_identities_on_floats(order):
    vals = np.array([1.5, -0.0, 0.0, -2.0, 1.5, np.inf, -2.0, 0.0, -np.inf, 1.5, 0.0], dtype=np.float32).view(np.uint32)
    nans = np.array([0x7FC00000, 0x7FC00001, 0x7FC00000, 0xFFC00000], dtype=np.uint32)
    a = np.concatenate([vals, nans, vals[::-1]])
    inv, keys, counts, first = gr.want_group(a, ol.F32, order)
    assert keys.size == 6 + 3                     # -inf, -2, -0.0, +0.0, 1.5, inf and three NaN bit patterns
    assert np.array_equal(keys[inv.astype(np.int64)], a)
    assert np.array_equal(np.bincount(inv.astype(np.int64), minlength=keys.size), counts)
    assert np.array_equal(a[first.astype(np.int64)], keys)
    for j in range(keys.size):
        assert first[j] == np.flatnonzero(a == keys[j])[0]
    k = ol.kdf_keys(keys, ol.F32, order)
    assert np.all(k[1:] > k[:-1])


def test_empty():
    inv, keys, counts, first = gr.want_group(np.zeros(0, dtype=np.uint32), ol.U32)
    assert inv.size == keys.size == counts.size == first.size == 0
